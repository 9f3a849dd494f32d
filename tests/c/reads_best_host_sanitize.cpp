// The host best match per read (bitnuc_amd/csrc/reads_best_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force
// read-by-read, query-by-query, window-by-window reference in (distance, query, offset) order: every k in 1..32, read lengths around k and the word
// size, 1 / 3 / 7 reads, 1 / 2 / 17 queries with junk above 2k, exactly sized heap buffers for the reads, the words, the queries and the three
// outputs (a guard after each output), ASCII (mixed case; an invalid byte planted: its buffer index, outputs untouched) and packed input with junk in
// every read's pad bits; a query duplicated at a higher index and a window planted twice in one read must give the lower query and offset.
#include "../../bitnuc_amd/csrc/reads_best_host.h"

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

static uint32_t ref_dist(const uint8_t *codes, size_t k, uint64_t query) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += codes[i] != ((query >> (2 * i)) & 3);
    return d;
}

int main() {
    const size_t counts[] = {1, 3, 7};
    const size_t nqs[] = {1, 2, 17};
    unsigned long long cases = 0;
    for (size_t k = 1; k <= 32; ++k) {
        const size_t lens[] = {k, k + 1, 31, 32, 33, 64, 65, 150};
        for (size_t L : lens) {
            if (L < k) continue;
            for (size_t count : counts) {
                const size_t n = L * count, wpr = (L + 31) / 32;
                std::vector<uint8_t> codes(n);
                for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                if (L >= 3 * k + 2) // read 0's first window again, later in the read: the first offset must win
                    for (size_t i = 0; i < k; ++i) codes[2 * k + 1 + i] = codes[i];
                uint8_t *ascii = (uint8_t *)malloc(n);
                for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
                uint64_t *words = (uint64_t *)malloc(count * wpr * 8);
                for (size_t r = 0; r < count; ++r) {
                    uint64_t *w = words + r * wpr;
                    memset(w, 0, wpr * 8);
                    for (size_t i = 0; i < L; ++i) w[i / 32] |= (uint64_t)codes[r * L + i] << (2 * (i % 32));
                    if (L % 32) w[wpr - 1] |= next_u64() & ~((1ull << (2 * (L % 32))) - 1); // junk in the pad bits
                }
                for (size_t nq : nqs) {
                    uint64_t *queries = (uint64_t *)malloc(nq * 8);
                    uint32_t *query = (uint32_t *)malloc((count + 1) * 4), *pos = (uint32_t *)malloc((count + 1) * 4);
                    uint8_t *dist = (uint8_t *)malloc(count + 1);
                    for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                    { // the last query: read 0's first window (junk above 2k kept); with 17 queries also at index 5, which must win
                        uint64_t w = 0;
                        for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[i] << (2 * i);
                        queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                        if (nq == 17) queries[5] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63);
                    }
                    std::vector<uint32_t> wq(count, 0xFFFFFFFFu), wp(count, 0xFFFFFFFFu), wd(count, 0xFF);
                    for (size_t r = 0; r < count; ++r)
                        for (size_t q = 0; q < nq; ++q)
                            for (size_t i = 0; i + k <= L; ++i) {
                                const uint32_t d = ref_dist(codes.data() + r * L + i, k, queries[q]);
                                if (d < wd[r]) wd[r] = d, wq[r] = (uint32_t)q, wp[r] = (uint32_t)i; // (q, i) ascend: strict improvements only
                            }
                    CHECK(wd[0] == 0 && wq[0] <= (nq == 17 ? 5u : (uint32_t)nq - 1), "the planted query"); // (a lower query may match elsewhere at a small k)
                    for (int form = 0; form < 2; ++form) {
                        query[count] = pos[count] = 0xC0FFEEu;
                        dist[count] = 0x5A;
                        if (form == 0) {
                            const long long bad = bitnuc_host::reads_hdist_best_small(ascii, L, count, k, queries, nq, query, pos, dist);
                            CHECK(bad == -1, "k %zu L %zu: bad %lld", k, L, bad);
                        } else {
                            bitnuc_host::reads_hdist_best_packed_small(words, L, count, k, queries, nq, query, pos, dist);
                        }
                        for (size_t r = 0; r < count; ++r)
                            CHECK(query[r] == wq[r] && pos[r] == wp[r] && dist[r] == wd[r], "form %d k %zu L %zu count %zu nq %zu read %zu: (%u, %u, %u) vs (%u, %u, %u)",
                                  form, k, L, count, nq, r, query[r], pos[r], (unsigned)dist[r], wq[r], wp[r], wd[r]);
                        CHECK(query[count] == 0xC0FFEEu && pos[count] == 0xC0FFEEu && dist[count] == 0x5A, "guard overwritten");
                        ++cases;
                    }
                    // an invalid byte: its index in the buffer, outputs untouched
                    const size_t at = (size_t)(next_u64() % n);
                    const uint8_t keep = ascii[at];
                    ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                    for (size_t r = 0; r <= count; ++r) query[r] = pos[r] = 0x77, dist[r] = 0x77;
                    const long long bad = bitnuc_host::reads_hdist_best_small(ascii, L, count, k, queries, nq, query, pos, dist);
                    CHECK(bad == (long long)at, "k %zu L %zu: bad %lld vs %zu", k, L, bad, at);
                    for (size_t r = 0; r <= count; ++r) CHECK(query[r] == 0x77 && pos[r] == 0x77 && dist[r] == 0x77, "outputs written on an invalid byte");
                    ascii[at] = keep;
                    free(queries);
                    free(query);
                    free(pos);
                    free(dist);
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
    printf("reads best host ok: %llu cases\n", cases);
    return 0;
}
