// reads_best2_host.h -- the best match and the runner-up per read below the host cutoff (bitnuc_reads_hdist_best2 / _best2_packed): for every read of a
// fixed-length batch the lexicographically smallest (distance, query, offset) over the queries and the windows that lie wholly inside the read, and
// the smallest one over the queries OTHER than that one's.  A running top-2 over distinct queries per read: the windows come in ascending order and
// every query's own minimum only falls, so the two smallest of the per-query minima are kept exactly.  Plain C++ (no HIP):
// tests/c/reads_best2_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "reads_best_host.h" // reads_best_fill; packed_window and window_dist through it

namespace bitnuc_host {

// (distance, query, offset) as one number: d << 58 | q << 32 | i, all-ones = none yet
struct ReadsTop2 { uint64_t best, second; };
constexpr uint64_t kReadsTop2None = ~0ull;
static inline uint32_t reads_top2_query(uint64_t key) { return (uint32_t)(key >> 32) & 0x3FFFFFFu; }

// window i's word w against every query
template <class Q>
static inline void reads_best2_window(uint64_t w, size_t i, size_t k, const Q *queries, size_t nq, ReadsTop2 *t) {
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t c = ((uint64_t)window_dist(w, queries[q], k) << 58) | ((uint64_t)q << 32) | (uint64_t)i;
        if (t->best != kReadsTop2None && reads_top2_query(t->best) == q) { // the winner's own query: a better window of it, never a runner-up
            if (c < t->best) t->best = c;
        } else if (c < t->best) { // a new winner: the old one is another query's minimum, and below the old runner-up
            t->second = t->best;
            t->best = c;
        } else if (c < t->second) { // (also a better window of the runner-up's own query)
            t->second = c;
        }
    }
}

static inline void reads_best2_store(uint64_t key, uint32_t *query, uint32_t *pos, uint8_t *dist) {
    if (key == kReadsTop2None) return; // the fill stays
    *query = reads_top2_query(key);
    *pos = (uint32_t)key;
    *dist = (uint8_t)(key >> 58);
}

// packed reads of read_len bases, ceil(read_len / 32) words each (1 <= k <= min(read_len, 32), nq >= 1); the bits above a read's last base are never
// part of a window.  One query: the runner-up is the fill.
template <class Q>
static inline void reads_hdist_best2_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, uint32_t *query,
                                                  uint32_t *pos, uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    reads_best_fill(count, query, pos, dist);
    reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        for (size_t i = 0; i + k <= read_len; ++i) reads_best2_window(packed_window(words + r * wpr, i, k), i, k, queries, nq, &t);
        reads_best2_store(t.best, query + r, pos + r, dist + r);
        reads_best2_store(t.second, query2 + r, pos2 + r, dist2 + r);
    }
}

// back-to-back ASCII reads of read_len bytes (1 <= k <= min(read_len, 32), nq >= 1): -1 with the outputs written, or the index of the first invalid
// byte of the buffer (all six outputs untouched)
template <class Q>
static inline long long reads_hdist_best2_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, uint32_t *query,
                                                uint32_t *pos, uint8_t *dist, uint32_t *query2, uint32_t *pos2, uint8_t *dist2) {
    for (size_t i = 0; i < count * read_len; ++i) {
        const unsigned u = reads[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    reads_best_fill(count, query, pos, dist);
    reads_best_fill(count, query2, pos2, dist2);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = reads + r * read_len;
        ReadsTop2 t{kReadsTop2None, kReadsTop2None};
        uint64_t w = 0;
        for (size_t i = 0; i < read_len; ++i) {
            const uint64_t code = ((s[i] >> 1) ^ (s[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
            w = (w >> 2) | (code << (2 * (k - 1)));                  // window i + 1 - k, base b at bits 2 b
            if (i + 1 >= k) reads_best2_window(w, i + 1 - k, k, queries, nq, &t);
        }
        reads_best2_store(t.best, query + r, pos + r, dist + r);
        reads_best2_store(t.second, query2 + r, pos2 + r, dist2 + r);
    }
    return -1;
}

} // namespace bitnuc_host
