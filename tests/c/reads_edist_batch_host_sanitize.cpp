// The host indel-tolerant anchored match per read of a RAGGED batch (bitnuc_amd/csrc/reads_edist_host.h: reads_edist_anchored_batch_small /
// _packed_small) under AddressSanitizer + UndefinedBehaviorSanitizer, against the plain dynamic programme on each read's own span: D[0][j] = 0,
// D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1), per read and query the smallest D[k][j] over the span and its first j,
// the best the first minimum over the queries, the runner-up the first minimum over the others; the span of a read written down from the definition of
// the admissible offsets (START: pos_lo <= i <= min(pos_hi, last); END: pos_lo <= last - i <= pos_hi, i >= 0), not with anchored_batch_window.
// k in {1, 2, 15, 16, 17, 31, 32}, ranges of 1, 2, 4 and 64 - k + 1 offsets from pos_lo 0 and 5, both anchors, reads of every length that gives another
// number of admissible offsets (0 included: empty reads, reads below k, reads too short for pos_lo), 1 / 2 / 9 queries, exact queries and patterns.
// Exactly sized heap buffers; every ASCII byte OUTSIDE the spans -- in front of and behind them, and every byte of a read without a window -- is 'N' and
// poisoned: the host form neither validates nor reads it.  The packed words are exactly sized too (a zero-length read has none) with junk in the pad
// bits.  An invalid byte planted inside a span: its buffer index, outputs untouched.  The second triple as NULL pointers: the best triple unchanged.
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

// the span of a read of `len` bases from the definition: its first base and its number of bases (0: no window)
static void span_of(size_t len, size_t k, int from_end, size_t lo, size_t hi, size_t *first, size_t *bases) {
    *first = *bases = 0;
    if (len < k) return;
    const long long last = (long long)(len - k);
    long long a, b;
    if (from_end) a = last - (long long)hi < 0 ? 0 : last - (long long)hi, b = last - (long long)lo;
    else a = (long long)lo, b = (long long)hi < last ? (long long)hi : last;
    if (a > b) return;
    *first = (size_t)a, *bases = (size_t)(b - a) + k;
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

struct Batch {
    std::vector<uint64_t> off, woff;
    std::vector<uint8_t> codes;
    uint8_t *ascii;
    uint64_t *words;
    size_t count;
};

template <class Q>
static void run_forms(const Batch &b, size_t k, int from_end, size_t lo, size_t hi, const Q *queries, size_t nq, const std::vector<uint32_t> *wq,
                      const std::vector<uint32_t> *wp, const std::vector<uint32_t> *wd, unsigned long long *cases) {
    const size_t count = b.count;
    for (int form = 0; form < 2; ++form)
        for (int second = 1; second >= 0; --second) {
            Six o(count);
            o.set(0, count, 0x11, 0x11);
            o.set(count, count + 1, 0xC0FFEEu, 0x5A);
            uint32_t *q2 = second ? o.q[1] : nullptr, *p2 = second ? o.p[1] : nullptr;
            uint8_t *d2 = second ? o.d[1] : nullptr;
            if (form == 0) {
                const long long bad = bitnuc_host::reads_edist_anchored_batch_small(b.ascii, b.off.data(), count, k, from_end, lo, hi, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                CHECK(bad == -1, "k %zu: bad %lld", k, bad);
            } else {
                bitnuc_host::reads_edist_anchored_batch_packed_small(b.words, b.woff.data(), b.off.data(), count, k, from_end, lo, hi, queries, nq, o.q[0], o.p[0], o.d[0], q2,
                                                                     p2, d2);
            }
            for (int j = 0; j <= second; ++j)
                for (size_t r = 0; r < count; ++r)
                    CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == wp[j][r] && o.d[j][r] == wd[j][r],
                          "kind %zu form %d rank %d k %zu end %d lo %zu hi %zu nq %zu read %zu (len %zu): (%u, %u, %u) vs (%u, %u, %u)", sizeof(Q), form, j, k, from_end, lo, hi,
                          nq, r, (size_t)(b.off[r + 1] - b.off[r]), o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], wq[j][r], wp[j][r], wd[j][r]);
            if (!second) CHECK(o.all(1, 0, count, 0x11, 0x11), "the second triple written through NULL's neighbours");
            CHECK(o.all(0, count, count + 1, 0xC0FFEEu, 0x5A), "guard overwritten");
            ++*cases;
        }
}

// the expected six outputs of `pats` (every query as a pattern) from the plain DP on each read's own span
static void expect(const Batch &b, size_t k, int from_end, size_t lo, size_t hi, const std::vector<PatternSets> &pats, std::vector<uint32_t> *wq,
                   std::vector<uint32_t> *wp, std::vector<uint32_t> *wd) {
    const size_t nq = pats.size();
    for (int j = 0; j < 2; ++j) wq[j].assign(b.count, 0xFFFFFFFFu), wp[j].assign(b.count, 0xFFFFFFFFu), wd[j].assign(b.count, 0xFF);
    std::vector<uint32_t> md(nq), mj(nq);
    for (size_t r = 0; r < b.count; ++r) {
        size_t first, bases;
        span_of((size_t)(b.off[r + 1] - b.off[r]), k, from_end, lo, hi, &first, &bases);
        if (!bases) continue;
        for (size_t q = 0; q < nq; ++q) ref_edist(b.codes.data() + b.off[r] + first, bases, k, pats[q], &md[q], &mj[q]);
        for (int j = 0; j < 2; ++j)
            for (size_t q = 0; q < nq; ++q)
                if ((j == 0 || q != wq[0][r]) && md[q] < wd[j][r]) wd[j][r] = md[q], wq[j][r] = (uint32_t)q, wp[j][r] = (uint32_t)first + mj[q];
    }
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    const size_t nqs[] = {1, 2, 9};
    unsigned long long cases = 0;
    for (size_t k : ks) {
        const size_t widths[] = {1, 2, 4, 64 - k + 1};
        for (size_t width : widths)
            for (size_t lo : {(size_t)0, (size_t)5})
                for (int from_end = 0; from_end < 2; ++from_end) {
                    const size_t hi = lo + width - 1, need = k + lo;
                    // lengths: empty, below k, k, around what pos_lo needs, one per number of admissible offsets, longer ones, an empty read last
                    std::vector<size_t> lens = {0, k - 1, k, need > 0 ? need - 1 : 0, 0};
                    for (size_t j = 0; j <= width + 1; ++j) lens.push_back(need + j);
                    lens.push_back(need + width + 37);
                    lens.push_back(150);
                    lens.push_back(0);
                    for (size_t i = lens.size(); i > 1; --i) std::swap(lens[i - 1], lens[next_u64() % i]);
                    Batch b;
                    b.count = lens.size();
                    b.off.assign(1, 0), b.woff.assign(1, 0);
                    for (size_t len : lens) b.off.push_back(b.off.back() + len), b.woff.push_back(b.woff.back() + (len + 31) / 32);
                    const size_t total = (size_t)b.off.back(), nwords = (size_t)b.woff.back();
                    b.codes.resize(total);
                    for (auto &c : b.codes) c = (uint8_t)(next_u64() & 3);
                    b.ascii = (uint8_t *)malloc(total ? total : 1);
                    b.words = (uint64_t *)malloc(nwords ? nwords * 8 : 8);
                    memset(b.ascii, 'N', total);
                    memset(b.words, 0, nwords * 8);
                    std::vector<size_t> span_at; // the buffer indices of the span bytes
                    for (size_t r = 0; r < b.count; ++r) {
                        size_t first, bases;
                        span_of(lens[r], k, from_end, lo, hi, &first, &bases);
                        for (size_t i = 0; i < bases; ++i) {
                            const size_t at = (size_t)b.off[r] + first + i;
                            b.ascii[at] = (uint8_t)("ACGT"[b.codes[at]] | ((next_u64() & 1) ? 0x20 : 0));
                            span_at.push_back(at);
                        }
                        uint64_t *w = b.words + b.woff[r];
                        for (size_t i = 0; i < lens[r]; ++i) w[i / 32] |= (uint64_t)b.codes[b.off[r] + i] << (2 * (i % 32));
                        if (lens[r] % 32) w[(lens[r] - 1) / 32] |= next_u64() & ~((1ull << (2 * (lens[r] % 32))) - 1); // junk in the pad bits
                    }
                    for (size_t i = 0; i < total; ++i) // outside the spans: off limits
                        if (b.ascii[i] == 'N') POISON(b.ascii + i, 1);
                    for (size_t nq : nqs) {
                        // exact queries: random; the last one a read's first span bases with one base DELETED when k >= 3 (an indel the DP must find)
                        std::vector<uint64_t> queries(nq);
                        for (auto &q : queries) q = next_u64();
                        if (!span_at.empty()) {
                            const size_t from0 = span_at[0];
                            size_t avail = 0;
                            while (avail < span_at.size() && span_at[avail] == from0 + avail) ++avail; // the first read's span
                            uint64_t w = 0;
                            for (size_t i = 0, from = 0; i < k; ++i, ++from) {
                                if (k >= 3 && i == k / 2) ++from;
                                w |= (uint64_t)b.codes[from0 + (from < avail ? from : avail - 1)] << (2 * i);
                            }
                            queries[nq - 1] = k == 32 ? w : (w | (queries[nq - 1] << (2 * k)));
                            if (nq == 9) queries[4] = queries[nq - 1] ^ (k == 32 ? 0 : 1ull << 63); // an equal duplicate at a lower index
                        }
                        std::vector<PatternSets> pats(nq);
                        for (size_t q = 0; q < nq; ++q) pats[q] = bitnuc_host::pattern_of_2bit(queries[q], k);
                        std::vector<uint32_t> wq[2], wp[2], wd[2];
                        expect(b, k, from_end, lo, hi, pats, wq, wp, wd);
                        run_forms(b, k, from_end, lo, hi, queries.data(), nq, wq, wp, wd, &cases);
                        std::vector<PatternSets> rnd(nq); // random sets; query 0 all-N, the last one with an empty position
                        for (auto &p : rnd)
                            for (int c = 0; c < 4; ++c) p.allow[c] = (uint32_t)next_u64() & (uint32_t)next_u64();
                        for (int c = 0; c < 4; ++c) {
                            rnd[0].allow[c] = ~0u;
                            if (nq > 1) rnd[nq - 1].allow[c] &= ~(1u << (k / 2));
                        }
                        expect(b, k, from_end, lo, hi, rnd, wq, wp, wd);
                        run_forms(b, k, from_end, lo, hi, rnd.data(), nq, wq, wp, wd, &cases);
                        if (!span_at.empty()) { // an invalid byte inside a span: its index in the buffer, all six outputs untouched
                            const size_t at = span_at[(size_t)(next_u64() % span_at.size())];
                            const uint8_t keep = b.ascii[at];
                            b.ascii[at] = (uint8_t)"Nn-x"[next_u64() & 3];
                            Six o(b.count);
                            o.set(0, b.count + 1, 0x77, 0x77);
                            const long long bad = bitnuc_host::reads_edist_anchored_batch_small(b.ascii, b.off.data(), b.count, k, from_end, lo, hi, queries.data(), nq, o.q[0],
                                                                                                o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
                            CHECK(bad == (long long)at, "k %zu: bad %lld vs %zu", k, bad, at);
                            CHECK(o.all(0, 0, b.count + 1, 0x77, 0x77), "outputs written on an invalid byte");
                            b.ascii[at] = keep;
                        }
                    }
                    UNPOISON(b.ascii, total);
                    free(b.ascii);
                    free(b.words);
                }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads edist batch host ok: %llu cases\n", cases);
    return 0;
}
