// The host indel-tolerant anchored match per read (bitnuc_amd/csrc/reads_edist_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against the
// plain dynamic programme: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1), per read and query the
// smallest D[k][j] over 1 <= j <= n and its first j, the best the first minimum over the queries, the runner-up the first minimum over the others.
// k in {1, 2, 15, 16, 17, 31, 32} (k = 32: no shift by 32 anywhere, UBSan watches), spans n in {k, k + 1, 31, 32, 33, 63, 64} where admissible, span
// starts that put the span inside one packed word and across one and two word boundaries, 1 / 3 / 7 reads, 1 / 2 / 3 / 9 queries, exact queries with
// junk above 2k and patterns (random sets, an all-N and an empty position among them).  Exactly sized heap buffers; every ASCII byte OUTSIDE the spans
// is 'N' and poisoned: the host form neither validates nor reads it.  An invalid byte planted inside a span: its buffer index, outputs untouched.  The
// second triple as NULL pointers: the best triple unchanged.  Packed input with junk in every read's pad bits.
#include "../../bitnuc_amd/csrc/reads_edist_host.h"

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

using bitnuc_host::PatternSets;

// the plain DP: the smallest D[k][j], 1 <= j <= n, and its first j
static void ref_edist(const uint8_t *t, size_t n, size_t k, const PatternSets &p, uint32_t *dist, uint32_t *j_of) {
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
    *dist = 0xFFFFFFFFu;
    for (size_t j = 1; j <= n; ++j)
        if (prev[j] < *dist) *dist = prev[j], *j_of = (uint32_t)j;
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

template <class Q>
static void run_forms(const uint8_t *ascii, const uint64_t *words, size_t L, size_t count, size_t k, size_t lo, size_t n, const Q *queries, size_t nq,
                      const std::vector<uint32_t> *wq, const std::vector<uint32_t> *wp, const std::vector<uint32_t> *wd, unsigned long long *cases) {
    for (int form = 0; form < 2; ++form)
        for (int second = 1; second >= 0; --second) {
            Six o(count);
            o.set(0, count, 0x11, 0x11);
            o.set(count, count + 1, 0xC0FFEEu, 0x5A);
            uint32_t *q2 = second ? o.q[1] : nullptr, *p2 = second ? o.p[1] : nullptr;
            uint8_t *d2 = second ? o.d[1] : nullptr;
            if (form == 0) {
                const long long bad = bitnuc_host::reads_edist_anchored_small(ascii, L, count, k, lo, n, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                CHECK(bad == -1, "k %zu L %zu: bad %lld", k, L, bad);
            } else {
                bitnuc_host::reads_edist_anchored_packed_small(words, L, count, k, lo, n, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
            }
            for (int j = 0; j <= second; ++j)
                for (size_t r = 0; r < count; ++r)
                    CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == wp[j][r] && o.d[j][r] == wd[j][r],
                          "kind %zu form %d rank %d k %zu L %zu lo %zu n %zu count %zu nq %zu read %zu: (%u, %u, %u) vs (%u, %u, %u)", sizeof(Q), form, j, k, L, lo, n, count,
                          nq, r, o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], wq[j][r], wp[j][r], wd[j][r]);
            if (!second) CHECK(o.all(1, 0, count, 0x11, 0x11), "the second triple written through NULL's neighbours");
            CHECK(o.all(0, count, count + 1, 0xC0FFEEu, 0x5A), "guard overwritten");
            ++*cases;
        }
}

// the expected six outputs of `pats` (every query as a pattern) from the plain DP
static void expect(const std::vector<uint8_t> &codes, size_t L, size_t count, size_t k, size_t lo, size_t n, const std::vector<PatternSets> &pats,
                   std::vector<uint32_t> *wq, std::vector<uint32_t> *wp, std::vector<uint32_t> *wd) {
    const size_t nq = pats.size();
    for (int j = 0; j < 2; ++j) wq[j].assign(count, 0xFFFFFFFFu), wp[j].assign(count, 0xFFFFFFFFu), wd[j].assign(count, 0xFF);
    std::vector<uint32_t> md(nq), mj(nq);
    for (size_t r = 0; r < count; ++r) {
        for (size_t q = 0; q < nq; ++q) ref_edist(codes.data() + r * L + lo, n, k, pats[q], &md[q], &mj[q]);
        for (int j = 0; j < 2; ++j)
            for (size_t q = 0; q < nq; ++q)
                if ((j == 0 || q != wq[0][r]) && md[q] < wd[j][r]) wd[j][r] = md[q], wq[j][r] = (uint32_t)q, wp[j][r] = (uint32_t)lo + mj[q];
    }
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    const size_t counts[] = {1, 3, 7};
    const size_t nqs[] = {1, 2, 3, 9};
    const size_t L = 150;
    unsigned long long cases = 0;
    for (size_t k : ks) {
        const size_t ns[] = {k, k + 1, 31, 32, 33, 63, 64};
        for (size_t n : ns) {
            if (n < k || n > 64) continue;
            const size_t los[] = {0, 5, 30, 63, L - n}; // inside word 0; across one boundary; across two (n >= 34 from 30 or 63)
            for (size_t lo : los) {
                if (lo + n > L) continue;
                for (size_t count : counts) {
                    const size_t total = L * count, wpr = (L + 31) / 32;
                    std::vector<uint8_t> codes(total);
                    for (size_t i = 0; i < total; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                    uint8_t *ascii = (uint8_t *)malloc(total);
                    for (size_t i = 0; i < total; ++i) {
                        const size_t at = i % L;
                        ascii[i] = at >= lo && at < lo + n ? (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0)) : (uint8_t)'N';
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
                        POISON(ascii + r * L + lo + n, L - lo - n);
                    }
                    for (size_t nq : nqs) {
                        // exact queries: random, the last one read 0's first k span bases with one base DELETED when k >= 3 (an indel the DP must find)
                        uint64_t *queries = (uint64_t *)malloc(nq * 8);
                        for (size_t q = 0; q < nq; ++q) queries[q] = next_u64();
                        {
                            uint64_t w = 0;
                            for (size_t i = 0, from = 0; i < k; ++i, ++from) {
                                if (k >= 3 && i == k / 2) ++from; // skip a span base
                                w |= (uint64_t)codes[lo + (from < n ? from : n - 1)] << (2 * i);
                            }
                            queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                            if (nq == 9) queries[4] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63); // an equal duplicate at a lower index
                        }
                        std::vector<PatternSets> pats(nq);
                        for (size_t q = 0; q < nq; ++q) pats[q] = bitnuc_host::pattern_of_2bit(queries[q], k);
                        std::vector<uint32_t> wq[2], wp[2], wd[2];
                        expect(codes, L, count, k, lo, n, pats, wq, wp, wd);
                        if (nq == 1) CHECK(wd[1][0] == 0xFF && wq[1][0] == 0xFFFFFFFFu, "one query: no runner-up");
                        run_forms(ascii, words, L, count, k, lo, n, queries, nq, wq, wp, wd, &cases);
                        // singleton patterns: the same outputs (junk above k in the sets)
                        std::vector<PatternSets> sing = pats;
                        if (k < 32)
                            for (auto &p : sing)
                                for (int c = 0; c < 4; ++c) p.allow[c] |= (uint32_t)next_u64() << k;
                        run_forms(ascii, words, L, count, k, lo, n, sing.data(), nq, wq, wp, wd, &cases);
                        // random sets; query 0 all-N, the last one with an empty position
                        std::vector<PatternSets> rnd(nq);
                        for (auto &p : rnd)
                            for (int c = 0; c < 4; ++c) p.allow[c] = (uint32_t)next_u64() & (uint32_t)next_u64();
                        for (int c = 0; c < 4; ++c) {
                            rnd[0].allow[c] = ~0u;
                            if (nq > 1) rnd[nq - 1].allow[c] &= ~(1u << (k / 2));
                        }
                        expect(codes, L, count, k, lo, n, rnd, wq, wp, wd);
                        CHECK(wd[0][0] == 0 && wq[0][0] == 0 && wp[0][0] == lo + k, "all-N: distance 0 at the first end");
                        run_forms(ascii, words, L, count, k, lo, n, rnd.data(), nq, wq, wp, wd, &cases);
                        // an invalid byte inside a span: its index in the buffer, all six outputs untouched
                        const size_t at = (size_t)(next_u64() % count) * L + lo + (size_t)(next_u64() % n);
                        const uint8_t keep = ascii[at];
                        ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                        Six o(count);
                        o.set(0, count + 1, 0x77, 0x77);
                        const long long bad = bitnuc_host::reads_edist_anchored_small(ascii, L, count, k, lo, n, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                        CHECK(bad == (long long)at, "k %zu: bad %lld vs %zu", k, bad, at);
                        CHECK(o.all(0, 0, count + 1, 0x77, 0x77), "outputs written on an invalid byte");
                        ascii[at] = keep;
                        free(queries);
                    }
                    UNPOISON(ascii, total);
                    free(ascii);
                    free(words);
                }
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads edist host ok: %llu cases\n", cases);
    return 0;
}
