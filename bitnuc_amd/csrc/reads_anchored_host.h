// reads_anchored_host.h -- the anchored best match and runner-up per read below the host cutoff (bitnuc_reads_hdist_anchored / _anchored_packed): as
// reads_best2_host.h, but over the offsets pos_lo .. pos_lo + offsets - 1 of every read only, and reading (and validating) only the span bytes
// [pos_lo, pos_lo + offsets + k - 1) of each read.  The running top-2 over distinct queries is reads_best2_host.h's.  Plain C++ (no HIP):
// tests/c/reads_anchored_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_best2_host.h" // ReadsTop2, reads_best2_window, reads_best2_store, reads_best_fill; packed_window through it

namespace bitnuc_host {

// the admissible offsets of a read: pos_lo <= i <= min(pos_hi, read_len - k).  false: none (k == 0, read_len < k or pos_lo beyond the last one)
static inline bool anchored_offsets(size_t read_len, size_t k, size_t pos_lo, size_t pos_hi, size_t *offsets) {
    if (k == 0 || read_len < k) return false;
    const size_t hi = pos_hi < read_len - k ? pos_hi : read_len - k;
    if (pos_lo > hi) return false;
    *offsets = hi - pos_lo + 1;
    return true;
}

static inline void anchored_store_top2(const ReadsTop2 &t, size_t r, uint32_t *query, uint32_t *pos, uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    reads_best2_store(t.best, query + r, pos + r, dist + r);
    if (query2) reads_best2_store(t.second, query2 + r, pos2 + r, dist2 + r);
}

// packed reads of read_len bases, ceil(read_len / 32) words each (1 <= k <= 32, offsets >= 1, pos_lo + offsets + k - 1 <= read_len, nq >= 1); query2 /
// pos2 / dist2 all NULL: the best triple only
template <class Q>
static inline void reads_hdist_anchored_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t offsets, const Q *queries,
                                                     size_t nq, uint32_t *query, uint32_t *pos, uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    reads_best_fill(count, query, pos, dist);
    if (query2) reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        for (size_t i = pos_lo; i < pos_lo + offsets; ++i) reads_best2_window(packed_window(words + r * wpr, i, k), i, k, queries, nq, &t);
        anchored_store_top2(t, r, query, pos, dist, query2, pos2, dist2);
    }
}

// back-to-back ASCII reads of read_len bytes (the same conditions): -1 with the outputs written, or the index of the first invalid byte, in buffer order,
// among the span bytes (outputs untouched).  Bytes outside the spans are never read.
template <class Q>
static inline long long reads_hdist_anchored_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t offsets, const Q *queries,
                                                   size_t nq, uint32_t *query, uint32_t *pos, uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    const size_t span = offsets + k - 1;
    for (size_t r = 0; r < count; ++r)
        for (size_t i = 0; i < span; ++i) {
            const unsigned u = reads[r * read_len + pos_lo + i] & 0xDFu;
            if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)(r * read_len + pos_lo + i);
        }
    reads_best_fill(count, query, pos, dist);
    if (query2) reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = reads + r * read_len + pos_lo;
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        uint64_t w = 0;
        for (size_t i = 0; i < span; ++i) {
            const uint64_t code = ((s[i] >> 1) ^ (s[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
            w = (w >> 2) | (code << (2 * (k - 1)));                  // window i + 1 - k of the span, base b at bits 2 b
            if (i + 1 >= k) reads_best2_window(w, pos_lo + i + 1 - k, k, queries, nq, &t);
        }
        anchored_store_top2(t, r, query, pos, dist, query2, pos2, dist2);
    }
    return -1;
}

} // namespace bitnuc_host
