// reads_edist_best_host.h -- the indel-tolerant best match and runner-up per read over the WHOLE read below the host cutoff (bitnuc_reads_edist_best /
// _packed / _batch / _batch_packed and their pattern twins): per read the smallest (edit distance, query, end) over the queries, the edit distance being
// the Levenshtein distance of the query to the best substring of the read, and the smallest over the queries other than the winner's.  reads_edist_host.h's
// edist_read (its edist_walk: Myers 1999 in Hyyro's form, one 32-bit column per (read, query)) over every base of the read: any read length, the end is a
// size_t until it is stored.  Plain C++ for both layouts and both query kinds; the tests' oracle is the plain DP, so the two are independent.  A read
// shorter than k is neither read nor validated and keeps the fill.  Plain C++ (no HIP): tests/c/reads_edist_best_host_sanitize.cpp runs them under ASan +
// UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_edist_host.h" // edist_read, edist_store_top2, edist_ascii_code, edist_packed_code, edist_first_invalid; reads_best_fill through it

namespace bitnuc_host {

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
        edist_store_top2(edist_read([&](size_t j) { return edist_packed_code(rw, j); }, read_len, k, 0, queries, nq), r, query, end, dist, query2, end2, dist2);
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
        edist_store_top2(edist_read([&](size_t j) { return edist_ascii_code(s[j]); }, read_len, k, 0, queries, nq), r, query, end, dist, query2, end2, dist2);
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
        edist_store_top2(edist_read([&](size_t j) { return edist_packed_code(rw, j); }, len, k, 0, queries, nq), r, query, end, dist, query2, end2, dist2);
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
        edist_store_top2(edist_read([&](size_t j) { return edist_ascii_code(s[j]); }, len, k, 0, queries, nq), r, query, end, dist, query2, end2, dist2);
    }
    return -1;
}

} // namespace bitnuc_host
