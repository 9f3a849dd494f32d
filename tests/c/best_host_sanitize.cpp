// The host best match (bitnuc_amd/csrc/scan_best_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force window-by-window
// reference: every k in 1..32, 1 / 2 / 17 queries with junk above 2k, exactly sized heap buffers for the queries, positions and distances (a guard
// after each), ASCII (mixed case; an invalid byte planted: outputs untouched) and packed input (junk above 2n); a window planted twice must give
// the first position.  And the row builders the device tables are made of (scan_mfma_host.h: scan_seg_row, scan_packed_row) against the host tables
// the shipped scans use (count_mfma_table, scan_packed_table).
#include "../../bitnuc_amd/csrc/scan_best_host.h"
#include "../../bitnuc_amd/csrc/scan_mfma_host.h"

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

static uint32_t ref_dist(const uint8_t *codes, size_t j, size_t k, uint64_t query) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += codes[j + i] != ((query >> (2 * i)) & 3);
    return d;
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
            if (n >= 3 * k + 2) // the first window again, later: the first position must win
                for (size_t i = 0; i < k; ++i) codes[2 * k + 1 + i] = codes[i];
            uint8_t *ascii = (uint8_t *)malloc(n);
            for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
            const size_t nw = (n + 31) / 32;
            uint64_t *words = (uint64_t *)malloc(nw * 8);
            memset(words, 0, nw * 8);
            for (size_t i = 0; i < n; ++i) words[i / 32] |= (uint64_t)codes[i] << (2 * (i % 32));
            if (n % 32) words[nw - 1] |= 0xA5A5A5A5A5A5A5A5ull & ~((1ull << (2 * (n % 32))) - 1);
            for (size_t nq : nqs) {
                uint64_t *queries = (uint64_t *)malloc(nq * 8);
                uint64_t *pos = (uint64_t *)malloc((nq + 1) * 8);
                uint8_t *dist = (uint8_t *)malloc(nq + 1);
                for (size_t q = 0; q < nq; ++q) {
                    queries[q] = next_u64();
                    if (q % 3 == 0) { // a window of the sequence (junk above 2k kept); query 0: the planted one
                        const size_t j = q == 0 ? 0 : (size_t)(next_u64() % (n - k + 1));
                        uint64_t w = 0;
                        for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[j + i] << (2 * i);
                        queries[q] = k == 32 ? w : (w | (queries[q] << (2 * k)));
                    }
                }
                std::vector<uint64_t> wpos(nq, ~0ull);
                std::vector<uint32_t> wdist(nq, 0xFF);
                for (size_t q = 0; q < nq; ++q)
                    for (size_t j = 0; j + k <= n; ++j) {
                        const uint32_t d = ref_dist(codes.data(), j, k, queries[q]);
                        if (d < wdist[q]) wdist[q] = d, wpos[q] = j;
                    }
                CHECK(wpos[0] == 0 && wdist[0] == 0, "the planted query");
                for (int form = 0; form < 2; ++form) {
                    pos[nq] = 0xC0FFEEull;
                    dist[nq] = 0x5A;
                    if (form == 0) {
                        const long long bad = bitnuc_host::kmer_hdist_best_small(ascii, n, k, queries, nq, pos, dist);
                        CHECK(bad == -1, "k %zu n %zu: bad %lld", k, n, bad);
                    } else {
                        bitnuc_host::kmer_hdist_best_packed_small(words, n, k, queries, nq, pos, dist);
                    }
                    for (size_t q = 0; q < nq; ++q)
                        CHECK(pos[q] == wpos[q] && dist[q] == wdist[q], "form %d k %zu n %zu q %zu: (%llu, %u) vs (%llu, %u)", form, k, n, q, (unsigned long long)pos[q],
                              (unsigned)dist[q], (unsigned long long)wpos[q], (unsigned)wdist[q]);
                    CHECK(pos[nq] == 0xC0FFEEull && dist[nq] == 0x5A, "guard overwritten");
                    ++cases;
                }
                // an invalid byte: its index, outputs untouched
                const size_t at = (size_t)(next_u64() % n);
                const uint8_t keep = ascii[at];
                ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                for (size_t q = 0; q <= nq; ++q) pos[q] = 0x77, dist[q] = 0x77;
                const long long bad = bitnuc_host::kmer_hdist_best_small(ascii, n, k, queries, nq, pos, dist);
                CHECK(bad == (long long)at, "k %zu n %zu: bad %lld vs %zu", k, n, bad, at);
                for (size_t q = 0; q <= nq; ++q) CHECK(pos[q] == 0x77 && dist[q] == 0x77, "outputs written on an invalid byte");
                ascii[at] = keep;
                free(queries);
                free(pos);
                free(dist);
            }
            free(ascii);
            free(words);
        }
    // the rows of the device tables are the rows of the host tables
    for (size_t k = 0; k <= 32; ++k)
        for (int rep = 0; rep < 8; ++rep) {
            const uint64_t query = next_u64();
            bitnuc_dev::CountMfmaTable ct;
            bitnuc_host::count_mfma_table(query, k, &ct);
            bitnuc_dev::PackedScanTable pt;
            bitnuc_host::scan_packed_table(query, k, &pt);
            uint32_t *row = (uint32_t *)malloc(16 * 4);
            for (int r = 0; r < 40; ++r) {
                bitnuc_host::scan_seg_row(query, k, r - 8, row);
                CHECK(memcmp(row, ct.w[r], 64) == 0, "scan_seg_row k %zu row %d", k, r);
            }
            for (int r = 0; r < 34; ++r) {
                bitnuc_host::scan_packed_row(query, k, r - 2, row);
                CHECK(memcmp(row, pt.w[r], 64) == 0, "scan_packed_row k %zu row %d", k, r);
            }
            free(row);
            ++cases;
        }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("best host ok: %llu cases\n", cases);
    return 0;
}
