// The host indel-tolerant hit list (bitnuc_amd/csrc/kmer_edist_host.h: kmer_edist_hits_small / kmer_edist_hits_packed_small) under AddressSanitizer +
// UndefinedBehaviorSanitizer, against the plain dynamic programme: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1,
// D[i][j-1] + 1), E(j) = D[k][j]; the hits are the j with E(j) <= tau in ascending order.
// k in {1, 2, 15, 16, 17, 31, 32} (k = 32: no shift by 32 anywhere, UBSan watches), n in {k, k + 1, 2k, 63, 64, 65, 200}, exact queries with junk above
// 2k and patterns, tau in {0, 1, k - 1, k, 2^32 - 1}, cap in {0, 1, total - 1, total, total + 1}, with and without hit_dist.  Exactly sized heap
// buffers for the sequence, the packed words and both outputs (cap == 0: NULL): one byte or word at or beyond cap is a report.  Packed input with junk
// above 2n.  An invalid byte: its index, outputs untouched.
#include "../../bitnuc_amd/csrc/kmer_edist_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static uint64_t rng_state = 0x13198A2E03707344ull;
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
static void run_case(size_t n, size_t k, const Q &query, const PatternSets &as_sets, const uint8_t *codes) {
    uint8_t *ascii = (uint8_t *)malloc(n);
    const size_t nw = (n + 31) / 32;
    uint64_t *words = (uint64_t *)malloc(nw * 8);
    for (size_t w = 0; w < nw; ++w) words[w] = 0;
    for (size_t j = 0; j < n; ++j) {
        ascii[j] = (uint8_t)("ACGTacgt"[codes[j] + 4 * (next_u64() % 3 == 0)]);
        words[j / 32] |= (uint64_t)codes[j] << (2 * (j % 32));
    }
    if (n % 32) words[nw - 1] |= next_u64() << (2 * (n % 32)); // junk above 2n
    const std::vector<uint32_t> e = ref_ends(codes, n, k, as_sets);
    const uint32_t taus[5] = {0u, 1u, (uint32_t)k - 1u, (uint32_t)k, 0xFFFFFFFFu};
    for (uint32_t tau : taus) {
        std::vector<uint64_t> want;
        for (size_t j = 0; j < n; ++j)
            if (e[j] <= tau) want.push_back(j + 1);
        const size_t total = want.size();
        const size_t caps[5] = {0, 1, total ? total - 1 : 0, total, total + 1};
        for (size_t cap : caps) {
            for (int with_dist = 0; with_dist < 2; ++with_dist) {
                for (int packed = 0; packed < 2; ++packed) {
                    uint64_t *end = cap ? (uint64_t *)malloc(cap * 8) : nullptr;
                    uint8_t *dist = cap && with_dist ? (uint8_t *)malloc(cap) : nullptr;
                    if (end) memset(end, 0x5A, cap * 8);
                    if (dist) memset(dist, 0x5A, cap);
                    uint64_t got = ~0ull;
                    if (packed) got = bitnuc_host::kmer_edist_hits_packed_small(words, n, k, query, tau, end, dist, cap);
                    else CHECK(bitnuc_host::kmer_edist_hits_small(ascii, n, k, query, tau, end, dist, cap, &got) == -1, "clean input reported invalid");
                    CHECK(got == total, "n %zu k %zu tau %u cap %zu packed %d: %llu hits, want %zu", n, k, tau, cap, packed, (unsigned long long)got, total);
                    for (size_t r = 0; r < cap; ++r) {
                        if (r < total) {
                            CHECK(end[r] == want[r] && (!dist || dist[r] == e[want[r] - 1]), "n %zu k %zu tau %u cap %zu packed %d: hit %zu", n, k, tau, cap, packed, r);
                        } else {
                            CHECK(end[r] == 0x5A5A5A5A5A5A5A5Aull && (!dist || dist[r] == 0x5A), "written behind the last hit");
                        }
                    }
                    free(end), free(dist);
                }
            }
        }
    }
    // an invalid byte: its index, nothing written
    const size_t at = next_u64() % n;
    ascii[at] = 'N';
    uint64_t end[2] = {0x5A5A5A5A5A5A5A5Aull, 0x5A5A5A5A5A5A5A5Aull}, got = 0x5A5A5A5A5A5A5A5Aull;
    uint8_t dist[2] = {0x5A, 0x5A};
    CHECK(bitnuc_host::kmer_edist_hits_small(ascii, n, k, query, (unsigned)k, end, dist, 2, &got) == (long long)at, "invalid byte index");
    CHECK(end[0] == 0x5A5A5A5A5A5A5A5Aull && end[1] == end[0] && dist[0] == 0x5A && dist[1] == 0x5A && got == 0x5A5A5A5A5A5A5A5Aull, "outputs touched");
    free(ascii), free(words);
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    for (size_t k : ks) {
        const size_t ns[] = {k, k + 1, 2 * k, 63, 64, 65, 200};
        for (size_t n : ns) {
            if (n < k) continue;
            uint8_t *codes = (uint8_t *)malloc(n);
            for (size_t j = 0; j < n; ++j) codes[j] = (uint8_t)(next_u64() & 3);
            const uint64_t query = next_u64(); // junk above 2k
            const PatternSets single = bitnuc_host::pattern_of_2bit(query, k);
            const size_t at = next_u64() % (n - k + 1); // a copy with, where it fits, one base dropped
            size_t o = at;
            const size_t drop = next_u64() % k;
            for (size_t i = 0; i < k && o < n; ++i) {
                if (i == drop && k > 2) continue;
                codes[o++] = (uint8_t)((query >> (2 * i)) & 3);
            }
            PatternSets pat;
            for (int c = 0; c < 4; ++c) pat.allow[c] = (uint32_t)next_u64() | (uint32_t)next_u64();
            run_case(n, k, query, single, codes);
            run_case(n, k, pat, pat, codes);
            free(codes);
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("kmer edist hits host ok\n");
    return 0;
}
