// scan_hist_host.h -- the mismatch histogram per query below the host cutoff (bitnuc_kmer_hdist_hist / _hist_packed and their pattern twins):
// hist[q * n_bins + d] = the number of windows j with window_dist(window j, queries[q], k) == d, d < n_bins; a window at n_bins or more is counted nowhere.
// Plain C++ (no HIP): tests/c/hist_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "host_word.h"    // packed_window
#include "pattern_host.h" // window_dist: exact queries (uint64_t) and patterns (PatternSets)

namespace bitnuc_host {

// window word w against every query
template <class Q>
static inline void hist_window(uint64_t w, size_t k, const Q *queries, size_t nq, size_t n_bins, uint64_t *hist) {
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t d = window_dist(w, queries[q], k);
        if (d < n_bins) ++hist[q * n_bins + d];
    }
}

// packed sequence of n bases (1 <= k <= min(n, 32)): hist[0 .. nq * n_bins) overwritten
template <class Q>
static inline void kmer_hdist_hist_packed_small(const uint64_t *words, size_t n, size_t k, const Q *queries, size_t nq, size_t n_bins, uint64_t *hist) {
    memset(hist, 0, nq * n_bins * sizeof(uint64_t));
    for (size_t j = 0; j + k <= n; ++j) hist_window(packed_window(words, j, k), k, queries, nq, n_bins, hist);
}

// ASCII sequence of n bytes (1 <= k <= min(n, 32)): -1 with hist[0 .. nq * n_bins) overwritten, or the index of the first invalid byte (hist untouched)
template <class Q>
static inline long long kmer_hdist_hist_small(const uint8_t *ref, size_t n, size_t k, const Q *queries, size_t nq, size_t n_bins, uint64_t *hist) {
    for (size_t i = 0; i < n; ++i) {
        const unsigned u = ref[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    memset(hist, 0, nq * n_bins * sizeof(uint64_t));
    uint64_t w = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t code = ((ref[i] >> 1) ^ (ref[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
        w = (w >> 2) | (code << (2 * (k - 1)));                      // window i + 1 - k, base b at bits 2 b
        if (i + 1 >= k) hist_window(w, k, queries, nq, n_bins, hist);
    }
    return -1;
}

} // namespace bitnuc_host
