// The host anchored best match and runner-up per read (bitnuc_amd/csrc/reads_anchored_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against
// a brute-force reference: per read and query the minimum distance over the offsets pos_lo .. pos_lo + offsets - 1 and its leftmost window, the best the
// first minimum over the queries, the runner-up the first minimum over the other queries.  k in {1, 2, 16, 31, 32}, read lengths around k, the word size
// and 150, start / interior / 3' anchors with 1, 2, 4 and the most offsets a span of 64 allows, 1 / 3 / 7 reads, 1 / 2 / 3 / 17 queries with junk above
// 2k.  Exactly sized heap buffers; every ASCII byte OUTSIDE the spans is 'N' and, where the sanitizer's granules allow, poisoned: the host form neither
// validates nor reads it.  An invalid byte planted inside a span: its buffer index, outputs untouched.  The second triple as NULL pointers: the best
// triple unchanged.  Packed input with junk in every read's pad bits.
#include "../../bitnuc_amd/csrc/reads_anchored_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

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
    bool all(int j0, size_t from, size_t to, uint32_t w, uint8_t b) const {
        for (int j = j0; j < 2; ++j)
            for (size_t r = from; r < to; ++r)
                if (q[j][r] != w || p[j][r] != w || d[j][r] != b) return false;
        return true;
    }
};

int main() {
    const size_t ks[] = {1, 2, 16, 31, 32};
    const size_t counts[] = {1, 3, 7};
    const size_t nqs[] = {1, 2, 3, 17};
    unsigned long long cases = 0;
    for (size_t k : ks) {
        const size_t lens[] = {k, k + 1, 33, 64, 65, 150};
        for (size_t L : lens) {
            if (L < k) continue;
            const size_t last = L - k, most = 64 - k + 1; // the last offset of a read; the most offsets a span of 64 holds
            // (pos_lo, pos_hi): start, interior and 3' anchors; pos_hi beyond the read's end is clamped
            std::vector<std::pair<size_t, size_t>> ranges;
            for (size_t w : {(size_t)1, (size_t)2, (size_t)4, most}) {
                if (w > last + 1) w = last + 1;
                ranges.push_back({0, w - 1});
                ranges.push_back({last + 1 - w, (size_t)-1});
                ranges.push_back({(last + 1 - w) / 2, (last + 1 - w) / 2 + w - 1});
                ranges.push_back({last + 1 - w, last + 5});
            }
            for (const auto &range : ranges) {
                const size_t lo = range.first;
                size_t offsets = 0;
                CHECK(bitnuc_host::anchored_offsets(L, k, lo, range.second, &offsets) && offsets >= 1 && lo + offsets - 1 <= last, "offsets");
                const size_t span = offsets + k - 1;
                CHECK(span <= 64, "span %zu", span);
                for (size_t count : counts) {
                    const size_t n = L * count, wpr = (L + 31) / 32;
                    std::vector<uint8_t> codes(n);
                    for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                    if (offsets >= 2) // read 0's first admissible window again at its last admissible offset
                        for (size_t i = 0; i < k; ++i) codes[lo + offsets - 1 + i] = codes[lo + i];
                    uint8_t *ascii = (uint8_t *)malloc(n);
                    for (size_t i = 0; i < n; ++i) {
                        const size_t at = i % L;
                        ascii[i] = at >= lo && at < lo + span ? (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0)) : (uint8_t)'N';
                    }
                    uint64_t *words = (uint64_t *)malloc(count * wpr * 8);
                    for (size_t r = 0; r < count; ++r) {
                        uint64_t *w = words + r * wpr;
                        memset(w, 0, wpr * 8);
                        for (size_t i = 0; i < L; ++i) w[i / 32] |= (uint64_t)codes[r * L + i] << (2 * (i % 32));
                        if (L % 32) w[wpr - 1] |= next_u64() & ~((1ull << (2 * (L % 32))) - 1); // junk in the pad bits
                    }
                    for (size_t r = 0; r < count; ++r) { // outside the spans: off limits
                        POISON(ascii + r * L, lo);
                        POISON(ascii + r * L + lo + span, L - lo - span);
                    }
                    for (size_t nq : nqs) {
                        uint64_t *queries = (uint64_t *)malloc(nq * 8);
                        for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                        { // the last query: read 0's first admissible window (junk above 2k kept); with 17 queries also at index 5
                            uint64_t w = 0;
                            for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[lo + i] << (2 * i);
                            queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                            if (nq == 17) queries[5] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63);
                        }
                        std::vector<uint32_t> wq[2], wp[2], wd[2];
                        for (int j = 0; j < 2; ++j) wq[j].assign(count, 0xFFFFFFFFu), wp[j].assign(count, 0xFFFFFFFFu), wd[j].assign(count, 0xFF);
                        std::vector<uint32_t> md(nq), mi(nq);
                        for (size_t r = 0; r < count; ++r) {
                            for (size_t q = 0; q < nq; ++q) {
                                md[q] = 0xFF;
                                for (size_t i = lo; i < lo + offsets; ++i) {
                                    const uint32_t d = ref_dist(codes.data() + r * L + i, k, queries[q]);
                                    if (d < md[q]) md[q] = d, mi[q] = (uint32_t)i;
                                }
                            }
                            for (int j = 0; j < 2; ++j)
                                for (size_t q = 0; q < nq; ++q)
                                    if ((j == 0 || q != wq[0][r]) && md[q] < wd[j][r]) wd[j][r] = md[q], wq[j][r] = (uint32_t)q, wp[j][r] = mi[q];
                        }
                        CHECK(wd[0][0] == 0 && (wq[0][0] != nq - 1 || wp[0][0] == lo), "the planted query, at the lower of its two offsets");
                        if (nq == 1) CHECK(wd[1][0] == 0xFF && wq[1][0] == 0xFFFFFFFFu, "one query: no runner-up");
                        for (int form = 0; form < 2; ++form)
                            for (int second = 1; second >= 0; --second) {
                                Six o(count);
                                o.set(0, count, 0x11, 0x11);
                                o.set(count, count + 1, 0xC0FFEEu, 0x5A);
                                uint32_t *q2 = second ? o.q[1] : nullptr, *p2 = second ? o.p[1] : nullptr;
                                uint8_t *d2 = second ? o.d[1] : nullptr;
                                if (form == 0) {
                                    const long long bad = bitnuc_host::reads_hdist_anchored_small(ascii, L, count, k, lo, offsets, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                                    CHECK(bad == -1, "k %zu L %zu: bad %lld", k, L, bad);
                                } else {
                                    bitnuc_host::reads_hdist_anchored_packed_small(words, L, count, k, lo, offsets, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                                }
                                for (int j = 0; j <= second; ++j)
                                    for (size_t r = 0; r < count; ++r)
                                        CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == wp[j][r] && o.d[j][r] == wd[j][r],
                                              "form %d rank %d k %zu L %zu lo %zu offsets %zu count %zu nq %zu read %zu: (%u, %u, %u) vs (%u, %u, %u)", form, j, k, L, lo, offsets,
                                              count, nq, r, o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], wq[j][r], wp[j][r], wd[j][r]);
                                if (!second) CHECK(o.all(1, 0, count, 0x11, 0x11), "the second triple written through NULL's neighbours");
                                CHECK(o.all(0, count, count + 1, 0xC0FFEEu, 0x5A), "guard overwritten");
                                ++cases;
                            }
                        // an invalid byte inside a span: its index in the buffer, all six outputs untouched
                        const size_t at = (size_t)(next_u64() % count) * L + lo + (size_t)(next_u64() % span);
                        const uint8_t keep = ascii[at];
                        ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                        Six o(count);
                        o.set(0, count + 1, 0x77, 0x77);
                        const long long bad = bitnuc_host::reads_hdist_anchored_small(ascii, L, count, k, lo, offsets, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                        CHECK(bad == (long long)at, "k %zu L %zu: bad %lld vs %zu", k, L, bad, at);
                        CHECK(o.all(0, 0, count + 1, 0x77, 0x77), "outputs written on an invalid byte");
                        ascii[at] = keep;
                        free(queries);
                    }
                    UNPOISON(ascii, n);
                    free(ascii);
                    free(words);
                }
            }
        }
    }
    { // no window
        size_t m = 0;
        CHECK(!bitnuc_host::anchored_offsets(10, 0, 0, 5, &m) && !bitnuc_host::anchored_offsets(10, 11, 0, 5, &m) && !bitnuc_host::anchored_offsets(10, 4, 7, (size_t)-1, &m),
              "empty ranges");
        CHECK(bitnuc_host::anchored_offsets(10, 4, 6, (size_t)-1, &m) && m == 1, "the last offset");
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads anchored host ok: %llu cases\n", cases);
    return 0;
}
