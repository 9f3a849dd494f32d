// scan_best_host.h -- the best match per query below the host cutoff (bitnuc_kmer_hdist_best / _best_packed): dist[q] = the smallest
// hdist_scalar(window j, queries[q], k) over the windows, pos[q] = the first window that attains it.  Plain C++ (no HIP):
// tests/c/best_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "host_word.h"    // packed_window
#include "pattern_host.h" // window_dist: exact queries (uint64_t) and patterns (PatternSets)

namespace bitnuc_host {

// window j's word w against every query: a strictly smaller distance takes the place (windows come in ascending order: the leftmost stays)
template <class Q>
static inline void best_window(uint64_t w, size_t j, size_t k, const Q *queries, size_t nq, uint64_t *pos, uint8_t *dist) {
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t d = window_dist(w, queries[q], k);
        if (d < dist[q]) dist[q] = (uint8_t)d, pos[q] = j;
    }
}

// packed sequence of n bases (1 <= k <= min(n, 32)): pos[0 .. nq) and dist[0 .. nq) overwritten
template <class Q>
static inline void kmer_hdist_best_packed_small(const uint64_t *words, size_t n, size_t k, const Q *queries, size_t nq, uint64_t *pos, uint8_t *dist) {
    memset(pos, 0xFF, nq * sizeof(uint64_t));
    memset(dist, 0xFF, nq);
    for (size_t j = 0; j + k <= n; ++j) best_window(packed_window(words, j, k), j, k, queries, nq, pos, dist);
}

// ASCII sequence of n bytes (1 <= k <= min(n, 32)): -1 with pos[0 .. nq) and dist[0 .. nq) overwritten, or the index of the first invalid byte (outputs
// untouched)
template <class Q>
static inline long long kmer_hdist_best_small(const uint8_t *ref, size_t n, size_t k, const Q *queries, size_t nq, uint64_t *pos, uint8_t *dist) {
    for (size_t i = 0; i < n; ++i) {
        const unsigned u = ref[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    memset(pos, 0xFF, nq * sizeof(uint64_t));
    memset(dist, 0xFF, nq);
    uint64_t w = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t code = ((ref[i] >> 1) ^ (ref[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
        w = (w >> 2) | (code << (2 * (k - 1)));                      // window i + 1 - k, base b at bits 2 b
        if (i + 1 >= k) best_window(w, i + 1 - k, k, queries, nq, pos, dist);
    }
    return -1;
}

} // namespace bitnuc_host
