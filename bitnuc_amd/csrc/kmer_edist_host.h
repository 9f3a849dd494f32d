// kmer_edist_host.h -- the indel-tolerant k-mer search along a reference below the host cutoff (bitnuc_kmer_edist_best / _count_multi / _hits, their _packed
// forms and their pattern twins): with E_q(j) the edit distance of query q to the best substring of the sequence that ends at base j (1 <= j <= n, the
// substring starts anywhere), dist[q] = min_j E_q(j) and end[q] = the first j that attains it; counts[q] = #{ j : E_q(j) <= taus[q] }.  The recurrence
// is reads_edist_host.h's edist_walk (with edist_peq and the code and validity helpers next to it), whose ends are size_t; the tests' oracle is the
// plain DP, so the two are independent.  Plain C++ (no HIP): tests/c/kmer_edist_host_sanitize.cpp runs them under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "reads_edist_host.h" // edist_peq, edist_walk, edist_ascii_code, edist_packed_code, edist_first_invalid

namespace bitnuc_host {

template <class Q, class CodeAt>
static inline void kmer_edist_best_codes(CodeAt code_at, size_t n, size_t k, const Q *queries, size_t nq, uint64_t *end, uint8_t *dist) {
    for (size_t q = 0; q < nq; ++q) {
        uint32_t bd = ~0u;
        uint64_t be = ~0ull;
        edist_walk(code_at, n, k, edist_peq(queries[q], k), [&](size_t j, uint32_t d) {
            if (d < bd) bd = d, be = j; // ends come in ascending order: the smallest stays
        });
        memcpy(end + q, &be, 8);
        dist[q] = (uint8_t)bd;
    }
}

template <class Q, class CodeAt>
static inline void kmer_edist_count_codes(CodeAt code_at, size_t n, size_t k, const Q *queries, const uint32_t *taus, size_t nq, uint64_t *counts) {
    for (size_t q = 0; q < nq; ++q) {
        uint64_t cnt = 0;
        const uint32_t tau = taus[q];
        edist_walk(code_at, n, k, edist_peq(queries[q], k), [&](size_t, uint32_t d) { cnt += d <= tau; });
        counts[q] = cnt;
    }
}

// packed sequence of n bases (1 <= k <= min(n, 32), nq >= 1): end[0 .. nq) and dist[0 .. nq) overwritten; bits above 2n of the last word are never read
template <class Q>
static inline void kmer_edist_best_packed_small(const uint64_t *words, size_t n, size_t k, const Q *queries, size_t nq, uint64_t *end, uint8_t *dist) {
    kmer_edist_best_codes([&](size_t j) { return edist_packed_code(words, j); }, n, k, queries, nq, end, dist);
}

// ASCII sequence of n bytes (the same conditions): -1 with the outputs overwritten, or the index of the first invalid byte among all n (outputs untouched)
template <class Q>
static inline long long kmer_edist_best_small(const uint8_t *ref, size_t n, size_t k, const Q *queries, size_t nq, uint64_t *end, uint8_t *dist) {
    const long long bad = edist_first_invalid(ref, n);
    if (bad >= 0) return bad;
    kmer_edist_best_codes([&](size_t j) { return edist_ascii_code(ref[j]); }, n, k, queries, nq, end, dist);
    return -1;
}

template <class Q>
static inline void kmer_edist_count_multi_packed_small(const uint64_t *words, size_t n, size_t k, const Q *queries, const uint32_t *taus, size_t nq,
                                                       uint64_t *counts) {
    kmer_edist_count_codes([&](size_t j) { return edist_packed_code(words, j); }, n, k, queries, taus, nq, counts);
}

template <class Q>
static inline long long kmer_edist_count_multi_small(const uint8_t *ref, size_t n, size_t k, const Q *queries, const uint32_t *taus, size_t nq,
                                                     uint64_t *counts) {
    const long long bad = edist_first_invalid(ref, n);
    if (bad >= 0) return bad;
    kmer_edist_count_codes([&](size_t j) { return edist_ascii_code(ref[j]); }, n, k, queries, taus, nq, counts);
    return -1;
}

// the hit list of one query: the ends j with D[k][j] <= tau in ascending order, the first `cap` of them kept (dist may be NULL); returns their number
template <class Q, class CodeAt>
static inline uint64_t kmer_edist_hits_codes(CodeAt code_at, size_t n, size_t k, const Q &query, unsigned tau, uint64_t *end, uint8_t *dist, size_t cap) {
    uint64_t hits = 0;
    edist_walk(code_at, n, k, edist_peq(query, k), [&](size_t j, uint32_t d) {
        if (d > tau) return;
        if (hits < cap) {
            const uint64_t e = j;
            memcpy(end + hits, &e, 8);
            if (dist) dist[hits] = (uint8_t)d;
        }
        ++hits;
    });
    return hits;
}

// packed sequence of n bases (1 <= k <= min(n, 32)): the number of hits; nothing is written at or beyond cap
template <class Q>
static inline uint64_t kmer_edist_hits_packed_small(const uint64_t *words, size_t n, size_t k, const Q &query, unsigned tau, uint64_t *end, uint8_t *dist,
                                                    size_t cap) {
    return kmer_edist_hits_codes([&](size_t j) { return edist_packed_code(words, j); }, n, k, query, tau, end, dist, cap);
}

// ASCII sequence of n bytes (the same conditions): -1 with *n_hits set, or the index of the first invalid byte among all n (outputs untouched)
template <class Q>
static inline long long kmer_edist_hits_small(const uint8_t *ref, size_t n, size_t k, const Q &query, unsigned tau, uint64_t *end, uint8_t *dist, size_t cap,
                                              uint64_t *n_hits) {
    const long long bad = edist_first_invalid(ref, n);
    if (bad >= 0) return bad;
    *n_hits = kmer_edist_hits_codes([&](size_t j) { return edist_ascii_code(ref[j]); }, n, k, query, tau, end, dist, cap);
    return -1;
}

} // namespace bitnuc_host
