// reads_edist_best_host.h -- the indel-tolerant best match and runner-up per read over the WHOLE read below the host cutoff (bitnuc_reads_edist_best /
// _packed / _batch / _batch_packed and their pattern twins): per read the smallest (edit distance, query, end) over the queries, the edit distance being
// the Levenshtein distance of the query to the best substring of the read, and the smallest over the queries other than the winner's.  The recurrence of
// reads_edist_host.h (Myers 1999 in Hyyro's form, one 32-bit column per (read, query)) walked over every base of the read: any read length, the end is a
// size_t until it is stored.  Plain C++ for both layouts and both query kinds; the tests' oracle is the plain DP, so the two are independent.  A read
// shorter than k is neither read nor validated and keeps the fill.  Plain C++ (no HIP): tests/c/reads_edist_best_host_sanitize.cpp runs them under ASan +
// UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_edist_host.h" // EdistPeq, edist_peq, edist_store_top2; ReadsTop2, reads_best_fill through it

namespace bitnuc_host {

// one read of n >= k bases (code(j) in 0 .. 3) against every query: the running top-2 over distinct queries (queries come in ascending order, one key
// each: d << 58 | q << 32 | end, end = the smallest j with the smallest D[k][j], one past the last aligned base; n < 2^32 - 1)
template <class Q, class Code>
static inline ReadsTop2 edist_best_read(Code code, size_t n, size_t k, const Q *queries, size_t nq) {
    ReadsTop2 t{kReadsTop2None, kReadsTop2None};
    const unsigned top = (unsigned)k - 1u;
    for (size_t q = 0; q < nq; ++q) {
        const EdistPeq p = edist_peq(queries[q], k);
        uint32_t pv = ~0u, mv = 0u, score = (uint32_t)k, best = ~0u;
        size_t end = 0;
        for (size_t j = 0; j < n; ++j) {
            const uint32_t eq = p.m[code(j)];
            const uint32_t xv = eq | mv;
            const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
            uint32_t ph = mv | ~(xh | pv);
            uint32_t mh = pv & xh;
            score += (ph >> top) & 1u;
            score -= (mh >> top) & 1u;
            if (score < best) best = score, end = j + 1;
            ph <<= 1; // no carry-in: D[0][j] = 0
            mh <<= 1;
            pv = mh | ~(xv | ph);
            mv = ph & xv;
        }
        const uint64_t c = ((uint64_t)best << 58) | ((uint64_t)q << 32) | (uint64_t)end;
        if (c < t.best) {
            t.second = t.best;
            t.best = c;
        } else if (c < t.second) {
            t.second = c;
        }
    }
    return t;
}

static inline uint8_t edist_ascii_code(uint8_t b) { return (uint8_t)(((b >> 1) ^ (b >> 2)) & 3u); } // A 0, C 1, G 2, T 3, either case
static inline uint8_t edist_packed_code(const uint64_t *words, size_t j) { return (uint8_t)((words[j / 32] >> (2 * (j % 32))) & 3u); }

// the first invalid byte of s[0, n), or -1
static inline long long edist_first_invalid(const uint8_t *s, size_t n) {
    for (size_t j = 0; j < n; ++j) {
        const unsigned u = s[j] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)j;
    }
    return -1;
}

// packed reads of read_len bases, ceil(read_len / 32) words each (1 <= k <= min(read_len, 32), nq >= 1); bits above a read's last base are never looked
// at.  query2 / end2 / dist2 all NULL: the best triple only
template <class Q>
static inline void reads_edist_best_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, uint32_t *query,
                                                 uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint64_t *rw = words + r * wpr;
        edist_store_top2(edist_best_read([&](size_t j) { return edist_packed_code(rw, j); }, read_len, k, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
}

// back-to-back ASCII reads of read_len bytes (the same conditions): -1 with the outputs written, or the index of the first invalid byte of the buffer
// (outputs untouched)
template <class Q>
static inline long long reads_edist_best_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, uint32_t *query,
                                               uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    const long long bad = edist_first_invalid(reads, count * read_len);
    if (bad >= 0) return bad;
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = reads + r * read_len;
        edist_store_top2(edist_best_read([&](size_t j) { return edist_ascii_code(s[j]); }, read_len, k, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
    return -1;
}

// ---- the RAGGED batch: reads behind reads_batch_host.h's validated tables.  A read of fewer than k bases keeps the fill; none of its bytes or words is
// read.

template <class Q>
static inline void reads_edist_best_batch_packed_small(const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                       const Q *queries, size_t nq, uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2,
                                                       uint8_t *dist2) {
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        if (len < k) continue;
        const uint64_t *rw = words + word_offsets[r];
        edist_store_top2(edist_best_read([&](size_t j) { return edist_packed_code(rw, j); }, len, k, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
}

// -1 with the outputs written, or the index of the first invalid byte, in buffer order, among the bytes of the reads of at least k bases (outputs
// untouched)
template <class Q>
static inline long long reads_edist_best_batch_small(const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const Q *queries, size_t nq,
                                                     uint32_t *query, uint32_t *end, uint8_t *dist, uint32_t *query2, uint32_t *end2, uint8_t *dist2) {
    for (size_t r = 0; r < count; ++r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        if (len < k) continue;
        const long long bad = edist_first_invalid(seq + offsets[r], len);
        if (bad >= 0) return (long long)offsets[r] + bad;
    }
    reads_best_fill(count, query, end, dist);
    if (query2) reads_best_fill(count, query2, end2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        if (len < k) continue;
        const uint8_t *s = seq + offsets[r];
        edist_store_top2(edist_best_read([&](size_t j) { return edist_ascii_code(s[j]); }, len, k, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
    return -1;
}

} // namespace bitnuc_host
