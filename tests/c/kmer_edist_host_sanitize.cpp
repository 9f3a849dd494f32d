// The host indel-tolerant k-mer search along a reference (bitnuc_amd/csrc/kmer_edist_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against
// the plain dynamic programme: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1), E(j) = D[k][j];
// best = the smallest E(j) and its first j, count = #{ j : E(j) <= tau }.
// k in {1, 2, 15, 16, 17, 31, 32} (k = 32: no shift by 32 anywhere, UBSan watches), n in {k, k + 1, 2k, 63, 64, 65, 200}, 1 / 2 / 5 queries, exact
// queries with junk above 2k and patterns (random sets, an all-N and an empty position among them), tau in {0, 1, k, 2^32 - 1}.  Exactly sized heap
// buffers for the sequence, the packed words and every output: one byte or word past them is a report.  Packed input with junk above 2n.  An invalid
// byte: its index, outputs untouched.
#include "../../bitnuc_amd/csrc/kmer_edist_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures < 20) {                         \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

using bitnuc_host::PatternSets;

static std::vector<uint32_t> ref_ends(const uint8_t *t, size_t n, size_t k, const PatternSets &p) {
    std::vector<uint32_t> prev(n + 1, 0), cur(n + 1);
    for (size_t i = 1; i <= k; ++i) {
        cur[0] = (uint32_t)i;
        for (size_t j = 1; j <= n; ++j) {
            const uint32_t sub = prev[j - 1] + (((p.allow[t[j - 1]] >> (i - 1)) & 1u) ? 0u : 1u);
            uint32_t v = sub < prev[j] + 1 ? sub : prev[j] + 1;
            if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
            cur[j] = v;
        }
        prev.swap(cur);
    }
    return std::vector<uint32_t>(prev.begin() + 1, prev.end());
}

template <class Q>
static void run_case(size_t n, size_t k, size_t nq, const Q *queries, const PatternSets *as_sets, const uint8_t *codes) {
    uint8_t *ascii = (uint8_t *)malloc(n);
    const size_t nw = (n + 31) / 32;
    uint64_t *words = (uint64_t *)malloc(nw * 8);
    for (size_t w = 0; w < nw; ++w) words[w] = 0;
    for (size_t j = 0; j < n; ++j) {
        ascii[j] = (uint8_t)("ACGTacgt"[codes[j] + 4 * (next_u64() % 3 == 0)]);
        words[j / 32] |= (uint64_t)codes[j] << (2 * (j % 32));
    }
    if (n % 32) words[nw - 1] |= next_u64() << (2 * (n % 32)); // junk above 2n
    uint64_t *end = (uint64_t *)malloc(nq * 8), *counts = (uint64_t *)malloc(nq * 8);
    uint8_t *dist = (uint8_t *)malloc(nq);
    uint32_t *taus = (uint32_t *)malloc(nq * 4);
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t pick[4] = {0u, 1u, (uint32_t)k, 0xFFFFFFFFu};
        taus[q] = pick[next_u64() % 4];
    }
    for (int packed = 0; packed < 2; ++packed) {
        memset(end, 0x5A, nq * 8), memset(dist, 0x5A, nq), memset(counts, 0x5A, nq * 8);
        if (packed) {
            bitnuc_host::kmer_edist_best_packed_small(words, n, k, queries, nq, end, dist);
            bitnuc_host::kmer_edist_count_multi_packed_small(words, n, k, queries, taus, nq, counts);
        } else {
            CHECK(bitnuc_host::kmer_edist_best_small(ascii, n, k, queries, nq, end, dist) == -1, "best: clean input reported invalid");
            CHECK(bitnuc_host::kmer_edist_count_multi_small(ascii, n, k, queries, taus, nq, counts) == -1, "count: clean input reported invalid");
        }
        for (size_t q = 0; q < nq; ++q) {
            const std::vector<uint32_t> e = ref_ends(codes, n, k, as_sets[q]);
            uint32_t bd = 0xFFFFFFFFu;
            uint64_t be = 0, cnt = 0;
            for (size_t j = 0; j < n; ++j) {
                if (e[j] < bd) bd = e[j], be = j + 1;
                cnt += e[j] <= taus[q];
            }
            CHECK(end[q] == be && dist[q] == bd && counts[q] == cnt, "n %zu k %zu q %zu packed %d: (%llu, %u, %llu) want (%llu, %u, %llu)", n, k, q, packed,
                  (unsigned long long)end[q], dist[q], (unsigned long long)counts[q], (unsigned long long)be, bd, (unsigned long long)cnt);
        }
    }
    // an invalid byte: its index, nothing written
    const size_t at = next_u64() % n;
    const uint8_t keep = ascii[at];
    ascii[at] = 'N';
    memset(end, 0x5A, nq * 8), memset(dist, 0x5A, nq), memset(counts, 0x5A, nq * 8);
    CHECK(bitnuc_host::kmer_edist_best_small(ascii, n, k, queries, nq, end, dist) == (long long)at, "best: invalid byte index");
    CHECK(bitnuc_host::kmer_edist_count_multi_small(ascii, n, k, queries, taus, nq, counts) == (long long)at, "count: invalid byte index");
    for (size_t q = 0; q < nq; ++q) CHECK(end[q] == 0x5A5A5A5A5A5A5A5Aull && dist[q] == 0x5A && counts[q] == 0x5A5A5A5A5A5A5A5Aull, "outputs touched");
    ascii[at] = keep;
    free(ascii), free(words), free(end), free(counts), free(dist), free(taus);
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    for (size_t k : ks) {
        const size_t ns[] = {k, k + 1, 2 * k, 63, 64, 65, 200};
        for (size_t n : ns) {
            if (n < k) continue;
            for (size_t nq : {(size_t)1, (size_t)2, (size_t)5}) {
                uint8_t *codes = (uint8_t *)malloc(n);
                for (size_t j = 0; j < n; ++j) codes[j] = (uint8_t)(next_u64() & 3);
                uint64_t *queries = (uint64_t *)malloc(nq * 8);
                std::vector<PatternSets> single(nq), pats(nq);
                for (size_t q = 0; q < nq; ++q) {
                    queries[q] = next_u64(); // junk above 2k
                    single[q] = bitnuc_host::pattern_of_2bit(queries[q], k);
                    const size_t at = next_u64() % (n - k + 1); // a copy with one base changed and, where it fits, one dropped
                    size_t o = at;
                    const size_t drop = next_u64() % k;
                    for (size_t i = 0; i < k && o < n; ++i) {
                        if (i == drop && k > 2) continue;
                        codes[o++] = (uint8_t)((queries[q] >> (2 * i)) & 3);
                    }
                    for (int c = 0; c < 4; ++c) pats[q].allow[c] = (uint32_t)next_u64() | (q == 1 ? 0xFFFFFFFFu : 0u); // 1: all-N
                    if (q == 2)
                        for (int c = 0; c < 4; ++c) pats[q].allow[c] &= ~(1u << (k / 2)); // an empty set
                }
                run_case(n, k, nq, queries, single.data(), codes);
                run_case(n, k, nq, pats.data(), pats.data(), codes);
                free(codes), free(queries);
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("kmer edist host ok\n");
    return 0;
}
