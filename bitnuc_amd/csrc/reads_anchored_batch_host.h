// reads_anchored_batch_host.h -- the anchored best match and runner-up per read of a RAGGED batch below the host cutoff (bitnuc_reads_hdist_anchored_batch /
// _anchored_batch_packed): reads_anchored_host.h behind reads_batch_host.h's tables, with a range per read -- counted from the read's start
// (BITNUC_ANCHOR_START) or, in bases behind the window, from its end (BITNUC_ANCHOR_END).  Only the span bytes of each read are read and validated.
// Plain C++ (no HIP): tests/c/reads_anchored_batch_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_anchored_host.h" // anchored_store_top2; ReadsTop2, reads_best2_window, reads_best_fill, packed_window through it
#include "reads_batch_host.h"    // the tables' validation and the chunk cut, for the callers

namespace bitnuc_host {

// offsets = pos_hi - pos_lo + 1 and span = offsets + k - 1 of a range, judged on the arguments alone, without overflow: a value that does not fit is
// SIZE_MAX.  pos_hi < pos_lo: an empty range, both 0.
static inline void anchored_batch_span(size_t k, size_t pos_lo, size_t pos_hi, size_t *offsets, size_t *span) {
    *offsets = *span = 0;
    if (pos_hi < pos_lo) return;
    const size_t d = pos_hi - pos_lo;
    *offsets = d == (size_t)-1 ? (size_t)-1 : d + 1;
    if (k == 0) { *span = *offsets == (size_t)-1 ? (size_t)-1 : *offsets - 1; return; }
    *span = *offsets > (size_t)-1 - (k - 1) ? (size_t)-1 : *offsets + (k - 1);
}

// the admissible offsets of a read of `len` bases: first .. first + n - 1 (n == 0: none).  k >= 1, pos_lo <= pos_hi.  last = len - k; START admits
// pos_lo <= i <= min(pos_hi, last); END admits the i = last - e with pos_lo <= e <= pos_hi and i >= 0.
struct AnchorWindow { size_t first, n; };
static inline AnchorWindow anchored_batch_window(size_t len, size_t k, int from_end, size_t pos_lo, size_t pos_hi) {
    if (len < k || len - k < pos_lo) return AnchorWindow{0, 0};
    const size_t room = len - k - pos_lo, width = pos_hi - pos_lo; // offsets beyond the first that the read / the range allow
    const size_t more = room < width ? room : width;
    return AnchorWindow{from_end ? room - more : pos_lo, more + 1};
}

// packed reads behind validated tables (1 <= k <= 32, pos_lo <= pos_hi, nq >= 1); query2 / pos2 / dist2 all NULL: the best triple only
template <class Q>
static inline void reads_hdist_anchored_batch_packed_small(const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                           int from_end, size_t pos_lo, size_t pos_hi, const Q *queries, size_t nq, uint32_t *query, uint32_t *pos,
                                                           uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    reads_best_fill(count, query, pos, dist);
    if (query2) reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        for (size_t i = w.first; i < w.first + w.n; ++i) reads_best2_window(packed_window(words + word_offsets[r], i, k), i, k, queries, nq, &t);
        anchored_store_top2(t, r, query, pos, dist, query2, pos2, dist2);
    }
}

// back-to-back ASCII reads behind a validated table (the same conditions): -1 with the outputs written, or the index of the first invalid byte, in buffer
// order, among the span bytes (outputs untouched).  Bytes outside the spans, and every byte of a read without a window, are never read.
template <class Q>
static inline long long reads_hdist_anchored_batch_small(const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int from_end, size_t pos_lo,
                                                         size_t pos_hi, const Q *queries, size_t nq, uint32_t *query, uint32_t *pos, uint8_t *dist, uint32_t *query2,
                                                         uint32_t *pos2, uint8_t *dist2) {
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        const size_t at = (size_t)offsets[r] + w.first;
        for (size_t i = 0; i < w.n + k - 1; ++i) {
            const unsigned u = seq[at + i] & 0xDFu;
            if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)(at + i);
        }
    }
    reads_best_fill(count, query, pos, dist);
    if (query2) reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        const uint8_t *s = seq + offsets[r] + w.first;
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        uint64_t x = 0;
        for (size_t i = 0; i < w.n + k - 1; ++i) {
            const uint64_t code = ((s[i] >> 1) ^ (s[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
            x = (x >> 2) | (code << (2 * (k - 1)));                  // window i + 1 - k of the span, base b at bits 2 b
            if (i + 1 >= k) reads_best2_window(x, w.first + i + 1 - k, k, queries, nq, &t);
        }
        anchored_store_top2(t, r, query, pos, dist, query2, pos2, dist2);
    }
    return -1;
}

} // namespace bitnuc_host
