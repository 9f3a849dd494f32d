// The host multi-query count (bitnuc_amd/csrc/scan_multi_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force
// window-by-window reference: every k in 1..32, 1 / 2 / 33 queries with junk above 2k and mixed thresholds {0, 1, k-1, k, k+1, 2^32-1}, exactly
// sized heap buffers for the queries, thresholds and counts (a guard word after the counts), ASCII (mixed case; an invalid byte planted: counts
// untouched) and packed input (junk above 2n).
#include "../../bitnuc_amd/csrc/scan_multi_host.h"

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

static uint32_t ref_dist(const uint8_t *codes, size_t j, size_t k, uint64_t query) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += codes[j + i] != ((query >> (2 * i)) & 3);
    return d;
}

int main() {
    const size_t sizes[] = {1, 2, 31, 32, 33, 64, 65, 100, 1000};
    const size_t nqs[] = {1, 2, 33};
    unsigned long long cases = 0;
    for (size_t k = 1; k <= 32; ++k)
        for (size_t n : sizes) {
            if (n < k) continue;
            std::vector<uint8_t> codes(n);
            for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
            uint8_t *ascii = (uint8_t *)malloc(n);
            for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
            const size_t nw = (n + 31) / 32;
            uint64_t *words = (uint64_t *)malloc(nw * 8);
            memset(words, 0, nw * 8);
            for (size_t i = 0; i < n; ++i) words[i / 32] |= (uint64_t)codes[i] << (2 * (i % 32));
            if (n % 32) words[nw - 1] |= 0xA5A5A5A5A5A5A5A5ull & ~((1ull << (2 * (n % 32))) - 1);
            for (size_t nq : nqs) {
                uint64_t *queries = (uint64_t *)malloc(nq * 8);
                uint32_t *taus = (uint32_t *)malloc(nq * 4);
                uint64_t *counts = (uint64_t *)malloc((nq + 1) * 8);
                const uint32_t pool[6] = {0u, 1u, (uint32_t)k - 1, (uint32_t)k, (uint32_t)k + 1, 0xFFFFFFFFu};
                for (size_t q = 0; q < nq; ++q) {
                    queries[q] = next_u64();
                    if (q % 3 == 0 && n >= k) { // a window of the sequence (junk above 2k kept)
                        const size_t j = (size_t)(next_u64() % (n - k + 1));
                        uint64_t w = 0;
                        for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[j + i] << (2 * i);
                        queries[q] = k == 32 ? w : (w | (queries[q] << (2 * k)));
                    }
                    taus[q] = pool[(q + k) % 6];
                }
                std::vector<uint64_t> want(nq, 0);
                for (size_t q = 0; q < nq; ++q)
                    for (size_t j = 0; j + k <= n; ++j) want[q] += ref_dist(codes.data(), j, k, queries[q]) <= taus[q];
                for (int form = 0; form < 2; ++form) {
                    counts[nq] = 0xC0FFEEull;
                    if (form == 0) {
                        const long long bad = bitnuc_host::kmer_hdist_count_multi_small(ascii, n, k, queries, taus, nq, counts);
                        CHECK(bad == -1, "k %zu n %zu: bad %lld", k, n, bad);
                    } else {
                        bitnuc_host::kmer_hdist_count_multi_packed_small(words, n, k, queries, taus, nq, counts);
                    }
                    for (size_t q = 0; q < nq; ++q) CHECK(counts[q] == want[q], "form %d k %zu n %zu q %zu: %llu vs %llu", form, k, n, q, (unsigned long long)counts[q], (unsigned long long)want[q]);
                    CHECK(counts[nq] == 0xC0FFEEull, "guard overwritten");
                    ++cases;
                }
                // an invalid byte: its index, counts untouched
                const size_t at = (size_t)(next_u64() % n);
                const uint8_t keep = ascii[at];
                ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                for (size_t q = 0; q <= nq; ++q) counts[q] = 0x77;
                const long long bad = bitnuc_host::kmer_hdist_count_multi_small(ascii, n, k, queries, taus, nq, counts);
                CHECK(bad == (long long)at, "k %zu n %zu: bad %lld vs %zu", k, n, bad, at);
                for (size_t q = 0; q <= nq; ++q) CHECK(counts[q] == 0x77, "counts written on an invalid byte");
                ascii[at] = keep;
                free(queries);
                free(taus);
                free(counts);
            }
            free(ascii);
            free(words);
        }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("multi host ok: %llu cases\n", cases);
    return 0;
}
