// The host hit lists (bitnuc_amd/csrc/scan_hits_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force
// window-by-window reference: every k in 1..32, tau in {0, 1, k-1, k, k+1, 2^32-1}, caps 0 / 1 / total-1 / total / total+5 with guard words after
// the cap in exactly-sized heap buffers, ASCII (mixed case, an invalid byte planted) and packed input (junk above 2n).
#include "../../bitnuc_amd/csrc/scan_hits_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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

template <class Run>
static void check_caps(const std::vector<uint64_t> &want_pos, const std::vector<uint8_t> &want_d, Run run, size_t k, unsigned tau, size_t n) {
    const size_t total = want_pos.size();
    const size_t caps[5] = {0, 1, total ? total - 1 : 0, total, total + 5};
    for (size_t cap : caps) {
        const size_t g = 4;
        uint64_t *pos = (uint64_t *)malloc((cap + g) * 8 + 8);
        uint8_t *dist = (uint8_t *)malloc(cap + g + 1);
        for (size_t i = 0; i < cap + g; ++i) pos[i] = 0xA5A5A5A5A5A5A5A5ull, dist[i] = 0xEE;
        for (int with_dist = 0; with_dist < 2; ++with_dist) {
            const uint64_t got = run(pos, with_dist ? dist : nullptr, cap);
            CHECK(got == total, "n %zu k %zu tau %u: %llu hits, want %zu", n, k, tau, (unsigned long long)got, total);
            const size_t m = cap < total ? cap : total;
            for (size_t i = 0; i < m; ++i) {
                CHECK(pos[i] == want_pos[i], "n %zu k %zu tau %u cap %zu: pos[%zu]", n, k, tau, cap, i);
                if (with_dist) CHECK(dist[i] == want_d[i], "n %zu k %zu tau %u cap %zu: dist[%zu]", n, k, tau, cap, i);
            }
            for (size_t i = cap; i < cap + g; ++i) CHECK(pos[i] == 0xA5A5A5A5A5A5A5A5ull && dist[i] == 0xEE, "written past cap %zu", cap);
        }
        free(pos);
        free(dist);
    }
}

int main() {
    const char *acgt = "ACGTacgt";
    for (size_t k = 1; k <= 32; ++k) {
        const size_t sizes[] = {k - 1, k, k + 1, 97, 300};
        for (size_t n : sizes) {
            for (int dense = 0; dense < 2; ++dense) {
                const uint64_t query = next_u64(); // junk above 2k
                std::vector<uint8_t> codes(n);
                for (size_t i = 0; i < n; ++i) codes[i] = dense && next_u64() % 10 ? (uint8_t)((query >> (2 * (i % k))) & 3) : (uint8_t)(next_u64() & 3);
                uint8_t *ascii = (uint8_t *)malloc(n + 1);
                for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)acgt[codes[i] + 4 * (next_u64() & 1)];
                const size_t nw = (n + 31) / 32;
                uint64_t *words = (uint64_t *)malloc(nw * 8 + 8);
                for (size_t w = 0; w < nw; ++w) words[w] = next_u64(); // junk above 2n
                for (size_t i = 0; i < n; ++i) {
                    words[i / 32] &= ~(3ull << (2 * (i % 32)));
                    words[i / 32] |= (uint64_t)codes[i] << (2 * (i % 32));
                }
                const unsigned taus[] = {0u, 1u, (unsigned)(k - 1), (unsigned)k, (unsigned)(k + 1), 0xFFFFFFFFu};
                for (unsigned tau : taus) {
                    std::vector<uint64_t> want_pos;
                    std::vector<uint8_t> want_d;
                    for (size_t j = 0; j + k <= n; ++j) {
                        const uint32_t d = ref_dist(codes.data(), j, k, query);
                        if (d <= tau) want_pos.push_back(j), want_d.push_back((uint8_t)d);
                    }
                    check_caps(want_pos, want_d, [&](uint64_t *pos, uint8_t *dist, size_t cap) {
                        return bitnuc_host::kmer_hdist_hits_packed_small(words, n, k, query, tau, pos, dist, cap);
                    }, k, tau, n);
                    check_caps(want_pos, want_d, [&](uint64_t *pos, uint8_t *dist, size_t cap) {
                        uint64_t nh = 0;
                        const long long bad = bitnuc_host::kmer_hdist_hits_small(ascii, n, k, query, tau, pos, dist, cap, &nh);
                        CHECK(bad == -1, "valid input reported invalid at %lld", bad);
                        return nh;
                    }, k, tau, n);
                }
                if (n >= k && n > 3) { // an invalid byte: its index, nothing written
                    const size_t at = (size_t)(next_u64() % n);
                    ascii[at] = 'N';
                    if (at + 1 < n) ascii[n - 1] = 'x';
                    uint64_t pos[2] = {7, 7}, nh = 99;
                    uint8_t dist[2] = {7, 7};
                    const long long bad = bitnuc_host::kmer_hdist_hits_small(ascii, n, k, query, 0xFFFFFFFFu, pos, dist, 2, &nh);
                    CHECK(bad == (long long)at && pos[0] == 7 && dist[0] == 7 && nh == 99, "invalid byte at %zu reported at %lld", at, bad);
                }
                free(ascii);
                free(words);
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("hits host ok\n");
    return 0;
}
