// The host mismatch histogram (bitnuc_amd/csrc/scan_hist_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force
// window-by-window reference: every k in 1..32, 1 / 2 / 17 queries with junk above 2k, every n_bins in 1..16, exactly sized heap buffers for the
// queries and the histogram (the sanitizer is the guard), ASCII (mixed case; an invalid byte planted: the histogram untouched) and packed input (junk
// above 2n), exact queries and patterns (random sets, empty ones and N among them).
#include "../../bitnuc_amd/csrc/scan_hist_host.h"

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
static uint32_t ref_pdist(const uint8_t *codes, size_t j, size_t k, const bitnuc_host::PatternSets &p) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += !((p.allow[codes[j + i]] >> i) & 1u);
    return d;
}

template <class Q, class Dist>
static void run_forms(const uint8_t *ascii, const uint64_t *words, const uint8_t *codes, size_t n, size_t k, const Q *queries, size_t nq, size_t n_bins,
                      Dist dist, unsigned long long *cases) {
    std::vector<uint64_t> want(nq * n_bins, 0);
    for (size_t q = 0; q < nq; ++q)
        for (size_t j = 0; j + k <= n; ++j) {
            const uint32_t d = dist(codes, j, k, queries[q]);
            if (d < n_bins) ++want[q * n_bins + d];
        }
    uint64_t *hist = (uint64_t *)malloc(nq * n_bins * 8); // exactly sized: a write past it is the sanitizer's to report
    for (int form = 0; form < 2; ++form) {
        memset(hist, 0x5A, nq * n_bins * 8);
        if (form == 0) {
            const long long bad = bitnuc_host::kmer_hdist_hist_small(ascii, n, k, queries, nq, n_bins, hist);
            CHECK(bad == -1, "k %zu n %zu: bad %lld", k, n, bad);
        } else {
            bitnuc_host::kmer_hdist_hist_packed_small(words, n, k, queries, nq, n_bins, hist);
        }
        for (size_t i = 0; i < nq * n_bins; ++i)
            CHECK(hist[i] == want[i], "form %d k %zu n %zu bins %zu cell %zu: %llu vs %llu", form, k, n, n_bins, i, (unsigned long long)hist[i],
                  (unsigned long long)want[i]);
        ++*cases;
    }
    free(hist);
}

int main() {
    const size_t sizes[] = {1, 2, 31, 32, 33, 64, 65, 100, 1000};
    const size_t nqs[] = {1, 2, 17};
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
                const size_t n_bins = 1 + (size_t)((k + n + nq) % 16); // every n_bins in 1..16 over the k and sizes
                uint64_t *queries = (uint64_t *)malloc(nq * 8);
                bitnuc_host::PatternSets *patterns = (bitnuc_host::PatternSets *)malloc(nq * sizeof(bitnuc_host::PatternSets));
                for (size_t q = 0; q < nq; ++q) {
                    queries[q] = next_u64();
                    const size_t j = (size_t)(next_u64() % (n - k + 1)); // a window of the sequence with a few bases changed (junk above 2k kept)
                    uint64_t w = 0;
                    for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[j + i] << (2 * i);
                    for (size_t c = next_u64() % (n_bins + 1); c > 0; --c) w ^= (1 + next_u64() % 3) << (2 * (next_u64() % k));
                    queries[q] = k == 32 ? w : (w | (queries[q] << (2 * k)));
                    patterns[q] = bitnuc_host::pattern_of_2bit(queries[q], k);
                    for (size_t i = 0; i < k; ++i) { // one position in four: a random set (empty and N among them)
                        if (next_u64() & 3) continue;
                        const unsigned set = (unsigned)(next_u64() & 15);
                        for (unsigned c = 0; c < 4; ++c) patterns[q].allow[c] = (patterns[q].allow[c] & ~(1u << i)) | (((set >> c) & 1u) << i);
                    }
                    for (unsigned c = 0; c < 4 && k < 32; ++c) patterns[q].allow[c] |= (uint32_t)next_u64() << k; // junk at positions >= k
                }
                run_forms(ascii, words, codes.data(), n, k, queries, nq, n_bins, ref_dist, &cases);
                run_forms(ascii, words, codes.data(), n, k, patterns, nq, n_bins, ref_pdist, &cases);
                // an invalid byte: its index, the histogram untouched
                const size_t at = (size_t)(next_u64() % n);
                const uint8_t keep = ascii[at];
                ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                uint64_t *hist = (uint64_t *)malloc(nq * n_bins * 8);
                for (size_t i = 0; i < nq * n_bins; ++i) hist[i] = 0x77;
                const long long bad = bitnuc_host::kmer_hdist_hist_small(ascii, n, k, queries, nq, n_bins, hist);
                CHECK(bad == (long long)at, "k %zu n %zu: bad %lld vs %zu", k, n, bad, at);
                for (size_t i = 0; i < nq * n_bins; ++i) CHECK(hist[i] == 0x77, "histogram written on an invalid byte");
                ascii[at] = keep;
                free(hist);
                free(queries);
                free(patterns);
            }
            free(ascii);
            free(words);
        }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("hist host ok: %llu cases\n", cases);
    return 0;
}
