// The host best match per read of a RAGGED batch (bitnuc_amd/csrc/reads_batch_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against a
// brute-force read-by-read, query-by-query, window-by-window reference in (distance, query, offset) order: every k in 1..32, batches of 1 / 4 / 9
// reads whose lengths mix 0, k - 1, k, k + 1, 31, 32, 33 and a random length up to 150, 1 / 2 / 17 queries with junk above 2k, exactly sized heap
// buffers for the bases, the words, both tables, the queries and the three outputs (a guard after each output), ASCII (mixed case; an invalid byte
// planted, also inside a read shorter than k: its buffer index, outputs untouched) and packed input with junk in every read's pad bits; then the table
// validation's findings in their order and the chunk cut.
#include "../../bitnuc_amd/csrc/reads_batch_host.h"

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

template <class T>
static T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); } // (a zero-size batch still gets a pointer the sanitizer watches)

int main() {
    const size_t counts[] = {1, 4, 9};
    const size_t nqs[] = {1, 2, 17};
    unsigned long long cases = 0;
    for (size_t k = 1; k <= 32; ++k) {
        const size_t pool[] = {0, k - 1, k, k + 1, 31, 32, 33, 0};
        for (size_t count : counts) {
            for (int rep = 0; rep < 3; ++rep) {
                uint64_t *offsets = exact<uint64_t>(count + 1), *woffsets = exact<uint64_t>(count + 1);
                offsets[0] = woffsets[0] = 0;
                for (size_t r = 0; r < count; ++r) {
                    const size_t pick = (size_t)(next_u64() % 9);
                    const size_t len = pick < 8 ? pool[pick] : (size_t)(next_u64() % 151);
                    offsets[r + 1] = offsets[r] + len;
                    woffsets[r + 1] = woffsets[r] + (len + 31) / 32;
                }
                const size_t n = (size_t)offsets[count], nw = (size_t)woffsets[count];
                std::vector<uint8_t> codes(n + 1);
                for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                uint8_t *ascii = exact<uint8_t>(n);
                for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
                uint64_t *words = exact<uint64_t>(nw);
                for (size_t r = 0; r < count; ++r) {
                    const size_t len = (size_t)(offsets[r + 1] - offsets[r]), wpr = (len + 31) / 32;
                    uint64_t *w = words + woffsets[r];
                    if (wpr) memset(w, 0, wpr * 8);
                    for (size_t i = 0; i < len; ++i) w[i / 32] |= (uint64_t)codes[offsets[r] + i] << (2 * (i % 32));
                    if (len % 32) w[wpr - 1] |= next_u64() & ~((1ull << (2 * (len % 32))) - 1); // junk in the pad bits
                }
                const bitnuc_host::BatchFault ok = bitnuc_host::batch_check_tables(offsets, woffsets, count);
                CHECK(ok.kind == 0, "valid tables refused: %d", ok.kind);
                size_t nwin = 0;
                for (size_t r = 0; r < count; ++r) nwin += offsets[r + 1] - offsets[r] >= k ? (size_t)(offsets[r + 1] - offsets[r]) - k + 1 : 0;
                CHECK(bitnuc_host::batch_windows(offsets, count, k) == nwin, "windows");
                for (size_t nq : nqs) {
                    uint64_t *queries = exact<uint64_t>(nq);
                    uint32_t *query = exact<uint32_t>(count + 1), *pos = exact<uint32_t>(count + 1);
                    uint8_t *dist = exact<uint8_t>(count + 1);
                    for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                    if (n >= k) { // one query is a window of the batch (it may straddle two reads: then no read may report distance 0 through it)
                        const size_t at = (size_t)(next_u64() % (n - k + 1));
                        uint64_t w = 0;
                        for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[at + i] << (2 * i);
                        queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                    }
                    std::vector<uint32_t> wq(count, 0xFFFFFFFFu), wp(count, 0xFFFFFFFFu), wd(count, 0xFF);
                    for (size_t r = 0; r < count; ++r)
                        for (size_t q = 0; q < nq; ++q)
                            for (size_t i = 0; offsets[r] + i + k <= offsets[r + 1]; ++i) {
                                const uint32_t d = ref_dist(codes.data() + offsets[r] + i, k, queries[q]);
                                if (d < wd[r]) wd[r] = d, wq[r] = (uint32_t)q, wp[r] = (uint32_t)i; // (q, i) ascend: strict improvements only
                            }
                    for (int form = 0; form < 2; ++form) {
                        query[count] = pos[count] = 0xC0FFEEu;
                        dist[count] = 0x5A;
                        if (form == 0) {
                            const long long bad = bitnuc_host::reads_hdist_best_batch_small(ascii, offsets, count, k, queries, nq, query, pos, dist);
                            CHECK(bad == -1, "k %zu: bad %lld", k, bad);
                        } else {
                            bitnuc_host::reads_hdist_best_batch_packed_small(words, woffsets, offsets, count, k, queries, nq, query, pos, dist);
                        }
                        for (size_t r = 0; r < count; ++r)
                            CHECK(query[r] == wq[r] && pos[r] == wp[r] && dist[r] == wd[r], "form %d k %zu count %zu nq %zu read %zu (len %zu): (%u, %u, %u) vs (%u, %u, %u)",
                                  form, k, count, nq, r, (size_t)(offsets[r + 1] - offsets[r]), query[r], pos[r], (unsigned)dist[r], wq[r], wp[r], wd[r]);
                        CHECK(query[count] == 0xC0FFEEu && pos[count] == 0xC0FFEEu && dist[count] == 0x5A, "guard overwritten");
                        ++cases;
                    }
                    if (n) { // an invalid byte anywhere, a read shorter than k included: its index in the buffer, outputs untouched
                        const size_t at = (size_t)(next_u64() % n);
                        const uint8_t keep = ascii[at];
                        ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                        for (size_t r = 0; r <= count; ++r) query[r] = pos[r] = 0x77, dist[r] = 0x77;
                        const long long bad = bitnuc_host::reads_hdist_best_batch_small(ascii, offsets, count, k, queries, nq, query, pos, dist);
                        CHECK(bad == (long long)at, "k %zu: bad %lld vs %zu", k, bad, at);
                        for (size_t r = 0; r <= count; ++r) CHECK(query[r] == 0x77 && pos[r] == 0x77 && dist[r] == 0x77, "outputs written on an invalid byte");
                        ascii[at] = keep;
                    }
                    free(queries);
                    free(query);
                    free(pos);
                    free(dist);
                }
                free(ascii);
                free(words);
                free(offsets);
                free(woffsets);
            }
        }
    }
    { // the table validation, in its order, on exactly sized tables
        uint64_t *off = exact<uint64_t>(5), *wo = exact<uint64_t>(5);
        const uint64_t good[5] = {0, 10, 10, 75, 107}, gw[5] = {0, 1, 1, 4, 5};
        auto reset = [&] { memcpy(off, good, sizeof good); memcpy(wo, gw, sizeof gw); };
        reset();
        CHECK(bitnuc_host::batch_check_tables(off, wo, 4).kind == 0 && bitnuc_host::batch_check_tables(off, nullptr, 4).kind == 0, "good tables");
        off[0] = 3, off[2] = 9, wo[3] = 9; // decreasing offsets come first
        bitnuc_host::BatchFault f = bitnuc_host::batch_check_tables(off, wo, 4);
        CHECK(f.kind == 1 && f.value == 2, "decreasing: %d %llu", f.kind, (unsigned long long)f.value);
        off[2] = 10;
        f = bitnuc_host::batch_check_tables(off, wo, 4);
        CHECK(f.kind == 2 && f.value == 0, "offsets[0]: %d", f.kind);
        off[0] = 0;
        f = bitnuc_host::batch_check_tables(off, wo, 4);
        CHECK(f.kind == 3 && f.value == 3, "word offsets: %d %llu", f.kind, (unsigned long long)f.value);
        reset();
        wo[0] = 1;
        f = bitnuc_host::batch_check_tables(off, wo, 4);
        CHECK(f.kind == 3 && f.value == 0, "word_offsets[0]");
        reset();
        off[4] = off[3] + 0xFFFFFFFFull, wo[4] = wo[3] + (0xFFFFFFFFull + 31) / 32;
        f = bitnuc_host::batch_check_tables(off, wo, 4);
        CHECK(f.kind == 4 && f.value == 0xFFFFFFFFull, "long read: %d", f.kind);
        off[4] = off[3] + 0xFFFFFFFEull, wo[4] = wo[3] + (0xFFFFFFFEull + 31) / 32;
        CHECK(bitnuc_host::batch_check_tables(off, wo, 4).kind == 0, "a read of 2^32 - 2 bases");
        // the chunk cut: the longest run of whole reads within the budget, at least one
        reset();
        auto size = [&](size_t a, size_t b) { return off[b] - off[a]; };
        CHECK(bitnuc_host::batch_chunk_end(0, 4, 10, size) == 2, "chunk: the empty read rides along");
        CHECK(bitnuc_host::batch_chunk_end(0, 4, 9, size) == 1, "chunk: at least one read");
        CHECK(bitnuc_host::batch_chunk_end(0, 4, 74, size) == 2 && bitnuc_host::batch_chunk_end(0, 4, 75, size) == 3, "chunk: the budget's edge");
        CHECK(bitnuc_host::batch_chunk_end(2, 4, 1000, size) == 4 && bitnuc_host::batch_chunk_end(3, 4, 1, size) == 4, "chunk: the end");
        free(off);
        free(wo);
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads batch host ok: %llu cases\n", cases);
    return 0;
}
