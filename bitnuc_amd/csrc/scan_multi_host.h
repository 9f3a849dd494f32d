// scan_multi_host.h -- the multi-query fused count below the host cutoff (bitnuc_kmer_hdist_count_multi / _multi_packed): counts[q] = the number of
// windows j with hdist_scalar(window j, queries[q], k) <= taus[q].  Plain C++ (no HIP): tests/c/multi_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "host_word.h"    // packed_window
#include "pattern_host.h" // window_dist: exact queries (uint64_t) and patterns (PatternSets)

namespace bitnuc_host {

// window word w against every query (Q: uint64_t, an exact query, or PatternSets)
template <class Q>
static inline void multi_count_window(uint64_t w, size_t k, const Q *queries, const uint32_t *taus, size_t nq, uint64_t *counts) {
    for (size_t q = 0; q < nq; ++q) counts[q] += window_dist(w, queries[q], k) <= taus[q];
}

// packed sequence of n bases (1 <= k <= min(n, 32)): counts[0 .. nq) overwritten
template <class Q>
static inline void kmer_hdist_count_multi_packed_small(const uint64_t *words, size_t n, size_t k, const Q *queries, const uint32_t *taus, size_t nq,
                                                       uint64_t *counts) {
    memset(counts, 0, nq * sizeof(uint64_t));
    for (size_t j = 0; j + k <= n; ++j) multi_count_window(packed_window(words, j, k), k, queries, taus, nq, counts);
}

// ASCII sequence of n bytes (1 <= k <= min(n, 32)): -1 with counts[0 .. nq) overwritten, or the index of the first invalid byte (counts untouched)
template <class Q>
static inline long long kmer_hdist_count_multi_small(const uint8_t *ref, size_t n, size_t k, const Q *queries, const uint32_t *taus, size_t nq,
                                                     uint64_t *counts) {
    for (size_t i = 0; i < n; ++i) {
        const unsigned u = ref[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    memset(counts, 0, nq * sizeof(uint64_t));
    uint64_t w = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t code = ((ref[i] >> 1) ^ (ref[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
        w = (w >> 2) | (code << (2 * (k - 1)));                      // window i + 1 - k, base b at bits 2 b
        if (i + 1 >= k) multi_count_window(w, k, queries, taus, nq, counts);
    }
    return -1;
}

} // namespace bitnuc_host
