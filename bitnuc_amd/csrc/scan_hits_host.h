// scan_hits_host.h -- the hit list of the sliding k-mer Hamming scan below the host cutoff (bitnuc_kmer_hdist_hits / _hits_packed):
// the windows j with hdist_scalar(window j, query, k) <= tau in ascending order, the first `cap` of them written to pos (and their distances to dist
// when it is not NULL), the number of all of them returned.  Plain C++ (no HIP): tests/c/hits_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "host_word.h"    // packed_window
#include "pattern_host.h" // window_dist: exact queries (uint64_t) and patterns (PatternSets)

namespace bitnuc_host {

// record hit number `hits` (window j, distance d) if it is below cap
static inline void hits_keep(uint64_t hits, size_t cap, uint64_t j, uint32_t d, uint64_t *pos, uint8_t *dist) {
    if (hits >= cap) return;
    pos[hits] = j;
    if (dist) dist[hits] = (uint8_t)d;
}

// packed sequence of n bases (1 <= k <= min(n, 32)); Q: uint64_t (an exact query) or PatternSets
template <class Q>
static inline uint64_t kmer_hdist_hits_packed_small(const uint64_t *words, size_t n, size_t k, const Q &query, unsigned tau, uint64_t *pos, uint8_t *dist,
                                                    size_t cap) {
    uint64_t hits = 0;
    for (size_t j = 0; j + k <= n; ++j) {
        const uint32_t d = window_dist(packed_window(words, j, k), query, k);
        if (d <= tau) hits_keep(hits++, cap, j, d, pos, dist);
    }
    return hits;
}

// ASCII sequence of n bytes (1 <= k <= min(n, 32)): -1 with *n_hits set, or the index of the first invalid byte (nothing written)
template <class Q>
static inline long long kmer_hdist_hits_small(const uint8_t *ref, size_t n, size_t k, const Q &query, unsigned tau, uint64_t *pos, uint8_t *dist,
                                              size_t cap, uint64_t *n_hits) {
    for (size_t i = 0; i < n; ++i) {
        const unsigned u = ref[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    uint64_t w = 0, hits = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t code = ((ref[i] >> 1) ^ (ref[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
        w = (w >> 2) | (code << (2 * (k - 1)));                      // window i + 1 - k, base b at bits 2 b
        if (i + 1 < k) continue;
        const uint32_t d = window_dist(w, query, k);
        if (d <= tau) hits_keep(hits++, cap, i + 1 - k, d, pos, dist);
    }
    *n_hits = hits;
    return -1;
}

} // namespace bitnuc_host
