// reads_edist_host.h -- the host side of the edit-distance family, and the indel-tolerant anchored best match and runner-up per read below the host cutoff
// (bitnuc_reads_edist_anchored / _packed, their _batch forms and their pattern twins).
// Shared by the three host headers of the family (this one, reads_edist_best_host.h, kmer_edist_host.h), each written once: edist_peq (a query's match
// masks, for both query kinds), edist_walk (THE column step: the same bit-parallel recurrence as the kernels' edist_step_device.h, Myers 1999 in Hyyro's
// form, one 32-bit column per (text, query), with a callback per end), edist_ascii_code / edist_packed_code, edist_first_invalid, and edist_read (one read's
// bases against every query: the top-2 over distinct queries) with edist_store_top2.
// The anchored match: per read the smallest (edit distance, query, end) over the queries, the edit distance being the Levenshtein distance of the query to
// the best substring of the read's span [pos_lo, pos_lo + n), and the smallest over the queries other than the winner's.  Plain C++ for both layouts and
// both query kinds; the tests' oracle is the plain DP, so the two are independent.  Only the span bytes of each read are read and validated.  Plain C++ (no
// HIP): tests/c/reads_edist_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_anchored_batch_host.h" // the ragged forms' window rule: AnchorWindow, anchored_batch_window
#include "reads_best2_host.h"          // ReadsTop2, reads_best2_store, reads_best_fill; PatternSets, pattern_of_2bit through scan_mfma_host.h

namespace bitnuc_host {

// Peq[c]: the positions < k of the query that base code c matches, by the query's kind
struct EdistPeq { uint32_t m[4]; };
static inline EdistPeq edist_peq(const PatternSets &p, size_t k) {
    const uint32_t ones = k >= 32 ? ~0u : ((1u << k) - 1u);
    return EdistPeq{{p.allow[0] & ones, p.allow[1] & ones, p.allow[2] & ones, p.allow[3] & ones}};
}
static inline EdistPeq edist_peq(uint64_t q, size_t k) { return edist_peq(pattern_of_2bit(q, k), k); }

// one query of 1 <= k <= 32 positions along n >= 1 bases (code_at(j) in 0 .. 3, 0-based): on_end(j + 1, D[k][j + 1]) for every j in ascending order -- THE
// column step of the host side, whatever the text is (a read's span, a whole read, a reference).  Bits at and above k of the column words are junk that
// never travels down; only bit k - 1 is tested.
template <class CodeAt, class OnEnd>
static inline void edist_walk(CodeAt code_at, size_t n, size_t k, const EdistPeq &p, OnEnd on_end) {
    uint32_t pv = ~0u, mv = 0u, score = (uint32_t)k;
    const unsigned top = (unsigned)k - 1u;
    for (size_t j = 0; j < n; ++j) {
        const uint32_t eq = p.m[code_at(j)];
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint32_t ph = mv | ~(xh | pv);
        uint32_t mh = pv & xh;
        score += (ph >> top) & 1u;
        score -= (mh >> top) & 1u;
        on_end(j + 1, score);
        ph <<= 1; // no carry-in: D[0][j] = 0
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
    }
}

static inline uint8_t edist_ascii_code(uint8_t b) { return (uint8_t)(((b >> 1) ^ (b >> 2)) & 3u); } // A 0, C 1, G 2, T 3, either case
static inline uint8_t edist_packed_code(const uint64_t *words, size_t j) { return (uint8_t)((words[j / 32] >> (2 * (j % 32))) & 3u); }

// the index of the first byte of s[0, n) outside ACGTacgt, or -1
static inline long long edist_first_invalid(const uint8_t *s, size_t n) {
    for (size_t j = 0; j < n; ++j) {
        const unsigned u = s[j] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)j;
    }
    return -1;
}

// n >= k bases of a read, the first of them its base `first`, against every query: the running top-2 over distinct queries (queries come in ascending
// order, one key each: d << 58 | q << 32 | end, end = first + the smallest j with the smallest D[k][j], one past the last aligned base; end < 2^32)
template <class Q, class CodeAt>
static inline ReadsTop2 edist_read(CodeAt code_at, size_t n, size_t k, size_t first, const Q *queries, size_t nq) {
    ReadsTop2 t{kReadsTop2None, kReadsTop2None};
    for (size_t q = 0; q < nq; ++q) {
        uint32_t best = ~0u;
        size_t end = 0;
        edist_walk(code_at, n, k, edist_peq(queries[q], k), [&](size_t j, uint32_t d) {
            if (d < best) best = d, end = j; // ends come in ascending order: the first stays
        });
        const uint64_t c = ((uint64_t)best << 58) | ((uint64_t)q << 32) | (uint64_t)(first + end);
        if (c < t.best) {
            t.second = t.best;
            t.best = c;
        } else if (c < t.second) {
            t.second = c;
        }
    }
    return t;
}

static inline void edist_store_top2(const ReadsTop2 &t, size_t r, uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    reads_best2_store(t.best, query + r, end + r, dist + r);
    if (query2) reads_best2_store(t.second, query2 + r, end2 + r, dist2 + r);
}

// packed reads of read_len bases, ceil(read_len / 32) words each (1 <= k <= 32, k <= n <= 64, pos_lo + n <= read_len, nq >= 1); query2 / end2 / dist2 all
// NULL: the best triple only
template <class Q>
static inline void reads_edist_anchored_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t n, const Q *queries, size_t nq,
                                                     uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint64_t *rw = words + r * wpr;
        edist_store_top2(edist_read([&](size_t j) { return edist_packed_code(rw, pos_lo + j); }, n, k, pos_lo, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
}

// back-to-back ASCII reads of read_len bytes (the same conditions): -1 with the outputs written, or the index of the first invalid byte, in buffer order,
// among the span bytes (outputs untouched).  Bytes outside the spans are never read.
template <class Q>
static inline long long reads_edist_anchored_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t n, const Q *queries, size_t nq,
                                                   uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    for (size_t r = 0; r < count; ++r) {
        const long long bad = edist_first_invalid(reads + r * read_len + pos_lo, n);
        if (bad >= 0) return (long long)(r * read_len + pos_lo) + bad;
    }
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = reads + r * read_len + pos_lo;
        edist_store_top2(edist_read([&](size_t j) { return edist_ascii_code(s[j]); }, n, k, pos_lo, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
    return -1;
}

// ---- the RAGGED batch (bitnuc_reads_edist_anchored_batch / _packed and their pattern twins): reads behind reads_batch_host.h's tables, a span per read.
// Read r's span is the bases the ragged Hamming form looks at: with (first, n) = anchored_batch_window(len_r, ...), read_r[first, first + n + k - 1);
// n == 0: no span, the fill, and the read is neither read nor validated.  Ends count from the read's start in both anchor modes.

// packed reads behind validated tables (1 <= k <= 32, pos_lo <= pos_hi, pos_hi - pos_lo + k <= 64, nq >= 1); query2 / end2 / dist2 all NULL: the best
// triple only
template <class Q>
static inline void reads_edist_anchored_batch_packed_small(const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                           int from_end, size_t pos_lo, size_t pos_hi, const Q *queries, size_t nq, uint32_t *query, uint32_t *end,
                                                           uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        const uint64_t *rw = words + word_offsets[r];
        edist_store_top2(edist_read([&](size_t j) { return edist_packed_code(rw, w.first + j); }, w.n + k - 1, k, w.first, queries, nq), r, query, end, dist, query2,
                         end2, dist2);
    }
}

// back-to-back ASCII reads behind a validated table (the same conditions): -1 with the outputs written, or the index of the first invalid byte, in buffer
// order, among the span bytes (outputs untouched).  Bytes outside the spans, and every byte of a read without a window, are never read.
template <class Q>
static inline long long reads_edist_anchored_batch_small(const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int from_end, size_t pos_lo,
                                                         size_t pos_hi, const Q *queries, size_t nq, uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2,
                                                         uint32_t *end2, uint8_t *dist2) {
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        const size_t at = (size_t)offsets[r] + w.first;
        const long long bad = edist_first_invalid(seq + at, w.n + k - 1);
        if (bad >= 0) return (long long)at + bad;
    }
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const AnchorWindow w = anchored_batch_window((size_t)(offsets[r + 1] - offsets[r]), k, from_end, pos_lo, pos_hi);
        if (!w.n) continue;
        const uint8_t *s = seq + offsets[r] + w.first;
        edist_store_top2(edist_read([&](size_t j) { return edist_ascii_code(s[j]); }, w.n + k - 1, k, w.first, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
    return -1;
}

} // namespace bitnuc_host
