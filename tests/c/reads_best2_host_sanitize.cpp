// The host best match and runner-up per read (bitnuc_amd/csrc/reads_best2_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a
// brute-force reference: per read and query the minimum distance and its leftmost window, the best the first minimum over the queries, the runner-up
// the first minimum over the other queries.  Every k in 1..32, read lengths around k and the word size, 1 / 3 / 7 reads, 1 / 2 / 3 / 17 queries with
// junk above 2k, exactly sized heap buffers for the reads, the words, the queries and the six outputs (a guard after each output), ASCII (mixed case;
// an invalid byte planted: its buffer index, outputs untouched) and packed input with junk in every read's pad bits; read 0's first window is planted
// again later in the read (the winner's own second window: never the runner-up) and, with 17 queries, as two equal queries (the second of them is the
// runner-up at the same distance and offset).
#include "../../bitnuc_amd/csrc/reads_best2_host.h"

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

static uint32_t ref_dist(const uint8_t *codes, size_t k, uint64_t query) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += codes[i] != ((query >> (2 * i)) & 3);
    return d;
}

struct Six {
    uint32_t *q[2], *p[2];
    uint8_t *d[2];
    explicit Six(size_t count) {
        for (int j = 0; j < 2; ++j) q[j] = (uint32_t *)malloc((count + 1) * 4), p[j] = (uint32_t *)malloc((count + 1) * 4), d[j] = (uint8_t *)malloc(count + 1);
    }
    ~Six() {
        for (int j = 0; j < 2; ++j) free(q[j]), free(p[j]), free(d[j]);
    }
    void set(size_t from, size_t to, uint32_t w, uint8_t b) {
        for (int j = 0; j < 2; ++j)
            for (size_t r = from; r < to; ++r) q[j][r] = p[j][r] = w, d[j][r] = b;
    }
    bool all(size_t from, size_t to, uint32_t w, uint8_t b) const {
        for (int j = 0; j < 2; ++j)
            for (size_t r = from; r < to; ++r)
                if (q[j][r] != w || p[j][r] != w || d[j][r] != b) return false;
        return true;
    }
};

int main() {
    const size_t counts[] = {1, 3, 7};
    const size_t nqs[] = {1, 2, 3, 17};
    unsigned long long cases = 0;
    for (size_t k = 1; k <= 32; ++k) {
        const size_t lens[] = {k, k + 1, 31, 32, 33, 64, 65, 150};
        for (size_t L : lens) {
            if (L < k) continue;
            for (size_t count : counts) {
                const size_t n = L * count, wpr = (L + 31) / 32;
                std::vector<uint8_t> codes(n);
                for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                if (L >= 3 * k + 2) // read 0's first window again, later in the read
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
                    for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                    { // the last query: read 0's first window (junk above 2k kept); with 17 queries also at index 5
                        uint64_t w = 0;
                        for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[i] << (2 * i);
                        queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                        if (nq == 17) queries[5] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63);
                    }
                    // the reference: per (read, query) minima, then the first minimum over the queries, twice
                    std::vector<uint32_t> wq[2], wp[2], wd[2];
                    for (int j = 0; j < 2; ++j) wq[j].assign(count, 0xFFFFFFFFu), wp[j].assign(count, 0xFFFFFFFFu), wd[j].assign(count, 0xFF);
                    std::vector<uint32_t> md(nq), mi(nq);
                    for (size_t r = 0; r < count; ++r) {
                        for (size_t q = 0; q < nq; ++q) {
                            md[q] = 0xFF;
                            for (size_t i = 0; i + k <= L; ++i) {
                                const uint32_t d = ref_dist(codes.data() + r * L + i, k, queries[q]);
                                if (d < md[q]) md[q] = d, mi[q] = (uint32_t)i;
                            }
                        }
                        for (int j = 0; j < 2; ++j)
                            for (size_t q = 0; q < nq; ++q)
                                if ((j == 0 || q != wq[0][r]) && md[q] < wd[j][r]) wd[j][r] = md[q], wq[j][r] = (uint32_t)q, wp[j][r] = mi[q];
                    }
                    CHECK(wd[0][0] == 0, "the planted query");
                    if (nq == 1) CHECK(wd[1][0] == 0xFF && wq[1][0] == 0xFFFFFFFFu, "one query: no runner-up");
                    if (nq == 17 && wq[0][0] == 5) // its equal duplicate at index 16 has the same minimum: the runner-up unless a lower query also matches
                        CHECK(wd[1][0] == 0 && (wq[1][0] < 16 || (wq[1][0] == 16 && wp[1][0] == wp[0][0])), "the duplicate is the runner-up");
                    for (int form = 0; form < 2; ++form) {
                        Six o(count);
                        o.set(0, count, 0x11, 0x11);
                        o.set(count, count + 1, 0xC0FFEEu, 0x5A);
                        if (form == 0) {
                            const long long bad = bitnuc_host::reads_hdist_best2_small(ascii, L, count, k, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                            CHECK(bad == -1, "k %zu L %zu: bad %lld", k, L, bad);
                        } else {
                            bitnuc_host::reads_hdist_best2_packed_small(words, L, count, k, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                        }
                        for (int j = 0; j < 2; ++j)
                            for (size_t r = 0; r < count; ++r)
                                CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == wp[j][r] && o.d[j][r] == wd[j][r],
                                      "form %d rank %d k %zu L %zu count %zu nq %zu read %zu: (%u, %u, %u) vs (%u, %u, %u)", form, j, k, L, count, nq, r, o.q[j][r], o.p[j][r],
                                      (unsigned)o.d[j][r], wq[j][r], wp[j][r], wd[j][r]);
                        CHECK(o.all(count, count + 1, 0xC0FFEEu, 0x5A), "guard overwritten");
                        ++cases;
                    }
                    // an invalid byte: its index in the buffer, all six outputs untouched
                    const size_t at = (size_t)(next_u64() % n);
                    const uint8_t keep = ascii[at];
                    ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                    Six o(count);
                    o.set(0, count + 1, 0x77, 0x77);
                    const long long bad = bitnuc_host::reads_hdist_best2_small(ascii, L, count, k, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                    CHECK(bad == (long long)at, "k %zu L %zu: bad %lld vs %zu", k, L, bad, at);
                    CHECK(o.all(0, count + 1, 0x77, 0x77), "outputs written on an invalid byte");
                    ascii[at] = keep;
                    free(queries);
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
    printf("reads best2 host ok: %llu cases\n", cases);
    return 0;
}
