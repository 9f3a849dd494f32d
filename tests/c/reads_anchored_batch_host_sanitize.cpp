// The host anchored best match and runner-up per read of a RAGGED batch (bitnuc_amd/csrc/reads_anchored_batch_host.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, against a brute-force reference written from the definition: per read its admissible offsets (START: pos_lo <= i <=
// min(pos_hi, last); END: pos_lo <= last - i <= pos_hi, i >= 0), per query the minimum distance over them and its leftmost window, the best the first
// minimum over the queries, the runner-up the first minimum over the other queries.  k in {1, 2, 16, 31, 32}, both anchors, ranges of 1, 2, 4 and the most
// offsets a span of 64 allows at pos_lo 0 and 3, batches whose lengths include 0, 1 .. k - 1, k, one base fewer than all offsets need, exactly enough and
// much longer, 1 / 2 / 3 / 17 queries with junk above 2k.  Exactly sized heap buffers; every ASCII byte OUTSIDE the spans -- the rest of a read, and every
// byte of a read without a window -- is 'N' and, where the sanitizer's granules allow, poisoned: the host form neither validates nor reads it.  An invalid
// byte planted inside a span: its buffer index, outputs untouched.  The second triple as NULL pointers: the best triple unchanged.  Packed input with
// junk in every read's pad bits.  The span arithmetic (anchored_batch_span) at its overflow edges.
#include "../../bitnuc_amd/csrc/reads_anchored_batch_host.h"

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

// the admissible offsets of a read, from the definition, by trying every offset
static void ref_window(size_t len, size_t k, int from_end, size_t lo, size_t hi, size_t *first, size_t *n) {
    *first = *n = 0;
    if (len < k) return;
    const size_t last = len - k;
    for (size_t i = 0; i <= last; ++i) {
        const size_t key = from_end ? last - i : i;
        if (key < lo || key > hi) continue;
        if (!*n) *first = i;
        ++*n;
    }
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
    const size_t nqs[] = {1, 2, 3, 17};
    unsigned long long cases = 0;
    for (size_t k : ks)
        for (int from_end = 0; from_end < 2; ++from_end)
            for (size_t lo : {(size_t)0, (size_t)3})
                for (size_t width : {(size_t)1, (size_t)2, (size_t)4, 64 - k + 1}) {
                    const size_t hi = lo + width - 1;
                    size_t offsets = 0, span = 0;
                    bitnuc_host::anchored_batch_span(k, lo, hi, &offsets, &span);
                    CHECK(offsets == width && span == width + k - 1 && span <= 64, "span %zu", span);
                    // the lengths: 0, 1 .. k - 1, k, around what all offsets need, much longer; then some random ones
                    std::vector<size_t> lens;
                    lens.push_back(0);
                    for (size_t L = 1; L <= k; L += (k > 4 ? k / 3 : 1)) lens.push_back(L);
                    lens.push_back(k - 1), lens.push_back(k);
                    for (size_t L = k + lo > 2 ? k + lo - 2 : 0; L <= k + lo + width + 1; ++L) lens.push_back(L);
                    lens.push_back(150), lens.push_back(0), lens.push_back(301);
                    for (int i = 0; i < 4; ++i) lens.push_back((size_t)(next_u64() % 90));
                    const size_t count = lens.size();
                    std::vector<uint64_t> off(count + 1, 0), woff(count + 1, 0);
                    for (size_t r = 0; r < count; ++r) off[r + 1] = off[r] + lens[r], woff[r + 1] = woff[r] + (lens[r] + 31) / 32;
                    const size_t n = (size_t)off[count], nw = (size_t)woff[count];
                    std::vector<uint8_t> codes(n + 1);
                    for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                    std::vector<size_t> first(count), num(count);
                    size_t planted = count; // a read with two offsets or more: its first admissible window again at its last admissible offset
                    for (size_t r = 0; r < count; ++r) {
                        ref_window(lens[r], k, from_end, lo, hi, &first[r], &num[r]);
                        const bitnuc_host::AnchorWindow w = bitnuc_host::anchored_batch_window(lens[r], k, from_end, lo, hi);
                        CHECK(w.n == num[r] && (!w.n || w.first == first[r]), "window of a read of %zu: (%zu, %zu) vs (%zu, %zu)", lens[r], w.first, w.n, first[r], num[r]);
                        if (planted == count && num[r] >= 2) {
                            planted = r;
                            for (size_t i = 0; i < k; ++i) codes[off[r] + first[r] + num[r] - 1 + i] = codes[off[r] + first[r] + i];
                        }
                    }
                    uint8_t *ascii = (uint8_t *)malloc(n ? n : 1);
                    memset(ascii, 'N', n);
                    for (size_t r = 0; r < count; ++r)
                        for (size_t i = 0; num[r] && i < num[r] + k - 1; ++i) {
                            const size_t at = (size_t)off[r] + first[r] + i;
                            ascii[at] = (uint8_t)("ACGT"[codes[at]] | ((next_u64() & 1) ? 0x20 : 0));
                        }
                    uint64_t *words = (uint64_t *)malloc(nw ? nw * 8 : 8);
                    for (size_t r = 0; r < count; ++r) {
                        uint64_t *w = words + woff[r];
                        const size_t wpr = (size_t)(woff[r + 1] - woff[r]);
                        memset(w, 0, wpr * 8);
                        for (size_t i = 0; i < lens[r]; ++i) w[i / 32] |= (uint64_t)codes[off[r] + i] << (2 * (i % 32));
                        if (lens[r] % 32) w[wpr - 1] |= next_u64() & ~((1ull << (2 * (lens[r] % 32))) - 1); // junk in the pad bits
                    }
                    for (size_t r = 0; r < count; ++r) { // outside the spans: off limits
                        const size_t s0 = num[r] ? first[r] : 0, s1 = num[r] ? first[r] + num[r] + k - 1 : 0;
                        POISON(ascii + off[r], s0);
                        POISON(ascii + off[r] + s1, lens[r] - s1);
                    }
                    for (size_t nq : nqs) {
                        uint64_t *queries = (uint64_t *)malloc(nq * 8);
                        for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                        if (planted < count) { // the last query: the planted read's first admissible window (junk above 2k kept); with 17 queries also at 5
                            uint64_t w = 0;
                            for (size_t i = 0; i < k; ++i) w |= (uint64_t)codes[off[planted] + first[planted] + i] << (2 * i);
                            queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                            if (nq == 17) queries[5] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63);
                        }
                        std::vector<uint32_t> wq[2], wp[2], wd[2];
                        for (int j = 0; j < 2; ++j) wq[j].assign(count, 0xFFFFFFFFu), wp[j].assign(count, 0xFFFFFFFFu), wd[j].assign(count, 0xFF);
                        std::vector<uint32_t> md(nq), mi(nq);
                        for (size_t r = 0; r < count; ++r) {
                            if (!num[r]) continue;
                            for (size_t q = 0; q < nq; ++q) {
                                md[q] = 0xFF;
                                for (size_t i = first[r]; i < first[r] + num[r]; ++i) {
                                    const uint32_t d = ref_dist(codes.data() + off[r] + i, k, queries[q]);
                                    if (d < md[q]) md[q] = d, mi[q] = (uint32_t)i;
                                }
                            }
                            for (int j = 0; j < 2; ++j)
                                for (size_t q = 0; q < nq; ++q)
                                    if ((j == 0 || q != wq[0][r]) && md[q] < wd[j][r]) wd[j][r] = md[q], wq[j][r] = (uint32_t)q, wp[j][r] = mi[q];
                        }
                        if (planted < count)
                            CHECK(wd[0][planted] == 0 && (wq[0][planted] != nq - 1 || wp[0][planted] == first[planted]), "the planted query, at the lower of its two offsets");
                        for (int form = 0; form < 2; ++form)
                            for (int second = 1; second >= 0; --second) {
                                Six o(count);
                                o.set(0, count, 0x11, 0x11);
                                o.set(count, count + 1, 0xC0FFEEu, 0x5A);
                                uint32_t *q2 = second ? o.q[1] : nullptr, *p2 = second ? o.p[1] : nullptr;
                                uint8_t *d2 = second ? o.d[1] : nullptr;
                                if (form == 0) {
                                    const long long bad = bitnuc_host::reads_hdist_anchored_batch_small(ascii, off.data(), count, k, from_end, lo, hi, queries, nq, o.q[0], o.p[0],
                                                                                                        o.d[0], q2, p2, d2);
                                    CHECK(bad == -1, "k %zu: bad %lld", k, bad);
                                } else {
                                    bitnuc_host::reads_hdist_anchored_batch_packed_small(words, woff.data(), off.data(), count, k, from_end, lo, hi, queries, nq, o.q[0], o.p[0],
                                                                                         o.d[0], q2, p2, d2);
                                }
                                for (int j = 0; j <= second; ++j)
                                    for (size_t r = 0; r < count; ++r)
                                        CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == wp[j][r] && o.d[j][r] == wd[j][r],
                                              "form %d rank %d k %zu end %d lo %zu hi %zu nq %zu read %zu (len %zu): (%u, %u, %u) vs (%u, %u, %u)", form, j, k, from_end, lo, hi, nq, r,
                                              lens[r], o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], wq[j][r], wp[j][r], wd[j][r]);
                                if (!second) CHECK(o.all(1, 0, count, 0x11, 0x11), "the second triple written through NULL's neighbours");
                                CHECK(o.all(0, count, count + 1, 0xC0FFEEu, 0x5A), "guard overwritten");
                                ++cases;
                            }
                        // an invalid byte inside a span: its index in the buffer, all six outputs untouched
                        size_t r = (size_t)(next_u64() % count);
                        while (!num[r]) r = (r + 1) % count;
                        const size_t at = (size_t)off[r] + first[r] + (size_t)(next_u64() % (num[r] + k - 1));
                        const uint8_t keep = ascii[at];
                        ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                        Six o(count);
                        o.set(0, count + 1, 0x77, 0x77);
                        const long long bad = bitnuc_host::reads_hdist_anchored_batch_small(ascii, off.data(), count, k, from_end, lo, hi, queries, nq, o.q[0], o.p[0], o.d[0],
                                                                                            o.q[1], o.p[1], o.d[1]);
                        CHECK(bad == (long long)at, "k %zu: bad %lld vs %zu", k, bad, at);
                        CHECK(o.all(0, 0, count + 1, 0x77, 0x77), "outputs written on an invalid byte");
                        ascii[at] = keep;
                        free(queries);
                    }
                    UNPOISON(ascii, n ? n : 1);
                    free(ascii);
                    free(words);
                }
    { // the span arithmetic: judged on the arguments alone, SIZE_MAX where a value does not fit
        const size_t M = (size_t)-1;
        size_t o, s;
        bitnuc_host::anchored_batch_span(5, 0, M, &o, &s);
        CHECK(o == M && s == M, "0 .. SIZE_MAX");
        bitnuc_host::anchored_batch_span(5, 1, M, &o, &s);
        CHECK(o == M && s == M, "1 .. SIZE_MAX: SIZE_MAX offsets, the span does not fit");
        bitnuc_host::anchored_batch_span(5, 6, M, &o, &s);
        CHECK(o == M - 5 && s == M - 1, "6 .. SIZE_MAX");
        bitnuc_host::anchored_batch_span(32, M - 32, M, &o, &s);
        CHECK(o == 33 && s == 64, "a span of 64 at the top of the range");
        bitnuc_host::anchored_batch_span(5, 7, 6, &o, &s);
        CHECK(o == 0 && s == 0, "an empty range");
        bitnuc_host::anchored_batch_span(0, 0, 0, &o, &s);
        CHECK(o == 1 && s == 0, "k == 0");
        const bitnuc_host::AnchorWindow w = bitnuc_host::anchored_batch_window(40, 8, 1, M - 3, M);
        CHECK(w.n == 0, "a range no read reaches");
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads anchored batch host ok: %llu cases\n", cases);
    return 0;
}
