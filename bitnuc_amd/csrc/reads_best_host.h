// reads_best_host.h -- the best match per read below the host cutoff (bitnuc_reads_hdist_best / _best_packed): for every read of a fixed-length batch
// the lexicographically smallest (distance, query, offset) over the queries and the windows that lie wholly inside the read.  Plain C++ (no HIP):
// tests/c/reads_best_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "host_word.h"    // packed_window
#include "pattern_host.h" // window_dist: exact queries (uint64_t) and patterns (PatternSets)

namespace bitnuc_host {

// window i's word w against every query: a smaller distance takes the place, an equal one only with a lower query (windows come in ascending order:
// of equal (distance, query) the leftmost stays)
template <class Q>
static inline void reads_best_window(uint64_t w, size_t i, size_t k, const Q *queries, size_t nq, uint32_t *query, uint32_t *pos, uint8_t *dist) {
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t d = window_dist(w, queries[q], k);
        if (d < *dist || (d == *dist && q < *query)) *dist = (uint8_t)d, *query = (uint32_t)q, *pos = (uint32_t)i;
    }
}

// every read without a window: UINT32_MAX, UINT32_MAX, 0xFF
static inline void reads_best_fill(size_t count, uint32_t *query, uint32_t *pos, uint8_t *dist) {
    memset(query, 0xFF, count * sizeof(uint32_t));
    memset(pos, 0xFF, count * sizeof(uint32_t));
    memset(dist, 0xFF, count);
}

// packed reads of read_len bases, ceil(read_len / 32) words each (1 <= k <= min(read_len, 32), nq >= 1); the bits above a read's last base are never
// part of a window
template <class Q>
static inline void reads_hdist_best_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq,
                                                 uint32_t *query, uint32_t *pos, uint8_t *dist) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    reads_best_fill(count, query, pos, dist);
    for (size_t r = 0; r < count; ++r)
        for (size_t i = 0; i + k <= read_len; ++i)
            reads_best_window(packed_window(words + r * wpr, i, k), i, k, queries, nq, query + r, pos + r, dist + r);
}

// back-to-back ASCII reads of read_len bytes (1 <= k <= min(read_len, 32), nq >= 1): -1 with the outputs written, or the index of the first invalid
// byte of the buffer (outputs untouched)
template <class Q>
static inline long long reads_hdist_best_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq,
                                               uint32_t *query, uint32_t *pos, uint8_t *dist) {
    for (size_t i = 0; i < count * read_len; ++i) {
        const unsigned u = reads[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    reads_best_fill(count, query, pos, dist);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = reads + r * read_len;
        uint64_t w = 0;
        for (size_t i = 0; i < read_len; ++i) {
            const uint64_t code = ((s[i] >> 1) ^ (s[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
            w = (w >> 2) | (code << (2 * (k - 1)));                  // window i + 1 - k, base b at bits 2 b
            if (i + 1 >= k) reads_best_window(w, i + 1 - k, k, queries, nq, query + r, pos + r, dist + r);
        }
    }
    return -1;
}

} // namespace bitnuc_host
