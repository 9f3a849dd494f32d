// The host indel-tolerant best match per read over the WHOLE read (bitnuc_amd/csrc/reads_edist_best_host.h: reads_edist_best_small / _packed_small /
// _batch_small / _batch_packed_small) under AddressSanitizer + UndefinedBehaviorSanitizer, against the plain dynamic programme over the whole read:
// D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1), per read and query the smallest D[k][j] and its first j, the
// best the first minimum over the queries, the runner-up the first minimum over the others.
// k in {1, 2, 15, 16, 17, 31, 32}, reads of k - 1, k, k + 1, 0, 63, 64, 65, 127, 128, 129, 150 and 257 bases, 1 / 2 / 5 queries, exact queries and patterns, both
// layouts.  Exactly sized heap buffers.  Ragged: the reads lie in a buffer with a gap of 'N' bytes in front of the batch, and EVERY byte outside the reads
// of at least k bases -- the gap and every byte of the reads shorter than k -- is poisoned: the host form neither validates nor reads it.  The packed words
// are exactly sized (a zero-length read has none), the words of reads shorter than k are poisoned, the pad bits hold junk.  An invalid byte planted
// inside a read: its buffer index, outputs untouched.  The second triple as NULL pointers: the best triple unchanged.
#include "../../bitnuc_amd/csrc/reads_edist_best_host.h"

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

static PatternSets sets_of(const PatternSets &p, size_t) { return p; }
static PatternSets sets_of(uint64_t q, size_t k) { return bitnuc_host::pattern_of_2bit(q, k); }

struct Six {
    uint32_t *q[2], *p[2];
    uint8_t *d[2];
    size_t count;
    explicit Six(size_t n) : count(n) {
        for (int j = 0; j < 2; ++j) {
            q[j] = (uint32_t *)malloc((n + 1) * 4), p[j] = (uint32_t *)malloc((n + 1) * 4), d[j] = (uint8_t *)malloc(n + 1);
            for (size_t r = 0; r <= n; ++r) q[j][r] = p[j][r] = r < n ? 0x11u : 0xC0FFEEu, d[j][r] = r < n ? 0x11 : 0x5A;
        }
    }
    ~Six() {
        for (int j = 0; j < 2; ++j) free(q[j]), free(p[j]), free(d[j]);
    }
    bool untouched(int j0) const {
        for (int j = j0; j < 2; ++j) {
            for (size_t r = 0; r < count; ++r)
                if (q[j][r] != 0x11u || p[j][r] != 0x11u || d[j][r] != 0x11) return false;
            if (q[j][count] != 0xC0FFEEu || p[j][count] != 0xC0FFEEu || d[j][count] != 0x5A) return false;
        }
        return true;
    }
};

static const char kLetters[] = "ACGTacgt";

template <class Q>
static void run(size_t k, const std::vector<size_t> &lens, const Q *queries, size_t nq, bool fixed, unsigned long long *cases) {
    const size_t count = lens.size(), gap = 5;
    std::vector<uint64_t> off(count + 1, 0), woff(count + 1, 0);
    for (size_t r = 0; r < count; ++r) off[r + 1] = off[r] + lens[r], woff[r + 1] = woff[r] + (lens[r] + 31) / 32;
    const size_t total = (size_t)off[count], nwords = (size_t)woff[count];
    uint8_t *buf = (uint8_t *)malloc(gap + total + 1);
    uint8_t *ascii = buf + gap; // offsets count from here: the gap in front is outside every read
    uint64_t *words = (uint64_t *)malloc((nwords + 1) * 8);
    std::vector<uint8_t> codes(total + 1);
    memset(buf, 'N', gap + total + 1);
    for (size_t w = 0; w < nwords; ++w) words[w] = next_u64(); // junk pad bits
    for (size_t r = 0; r < count; ++r)
        for (size_t j = 0; j < lens[r]; ++j) {
            const unsigned c = (unsigned)(next_u64() >> 60) & 3u;
            codes[off[r] + j] = (uint8_t)c;
            if (lens[r] >= k) ascii[off[r] + j] = (uint8_t)kLetters[c + 4 * ((next_u64() >> 33) & 1u)];
            uint64_t &w = words[woff[r] + j / 32];
            w = (w & ~(3ull << (2 * (j % 32)))) | ((uint64_t)c << (2 * (j % 32)));
        }
    // expected
    std::vector<uint32_t> wq[2], we[2], wd[2];
    for (int j = 0; j < 2; ++j) wq[j].assign(count, 0xFFFFFFFFu), we[j].assign(count, 0xFFFFFFFFu), wd[j].assign(count, 0xFFu);
    for (size_t r = 0; r < count; ++r) {
        if (lens[r] < k) continue;
        std::vector<uint32_t> d(nq), e(nq);
        for (size_t q = 0; q < nq; ++q) ref_edist(codes.data() + off[r], lens[r], k, sets_of(queries[q], k), &d[q], &e[q]);
        size_t b = 0;
        for (size_t q = 1; q < nq; ++q)
            if (d[q] < d[b]) b = q;
        wq[0][r] = (uint32_t)b, we[0][r] = e[b], wd[0][r] = d[b];
        size_t s = nq;
        for (size_t q = 0; q < nq; ++q)
            if (q != b && (s == nq || d[q] < d[s])) s = q;
        if (s != nq) wq[1][r] = (uint32_t)s, we[1][r] = e[s], wd[1][r] = d[s];
    }
    // poison: the gap, the byte behind the batch, every byte and word of a read shorter than k
    POISON(buf, gap);
    POISON(ascii + total, 1);
    POISON(words + nwords, 8);
    for (size_t r = 0; r < count; ++r)
        if (lens[r] < k) {
            POISON(ascii + off[r], lens[r]);
            POISON(words + woff[r], 8 * (size_t)(woff[r + 1] - woff[r]));
        }
    for (int form = 0; form < 2; ++form)
        for (int second = 1; second >= 0; --second) {
            Six o(count);
            uint32_t *q2 = second ? o.q[1] : nullptr, *p2 = second ? o.p[1] : nullptr;
            uint8_t *d2 = second ? o.d[1] : nullptr;
            long long bad = -1;
            if (fixed) {
                if (form == 0) bad = bitnuc_host::reads_edist_best_small(ascii, lens[0], count, k, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                else bitnuc_host::reads_edist_best_packed_small(words, lens[0], count, k, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
            } else {
                if (form == 0) bad = bitnuc_host::reads_edist_best_batch_small(ascii, off.data(), count, k, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
                else bitnuc_host::reads_edist_best_batch_packed_small(words, woff.data(), off.data(), count, k, queries, nq, o.q[0], o.p[0], o.d[0], q2, p2, d2);
            }
            CHECK(bad == -1, "k %zu form %d: clean input reported invalid at %lld", k, form, bad);
            for (int j = 0; j <= second; ++j)
                for (size_t r = 0; r < count; ++r)
                    CHECK(o.q[j][r] == wq[j][r] && o.p[j][r] == we[j][r] && o.d[j][r] == (uint8_t)wd[j][r],
                          "k %zu nq %zu form %d fixed %d triple %d read %zu (len %zu): got (%u, %u, %u) want (%u, %u, %u)", k, nq, form, (int)fixed, j, r, lens[r],
                          o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], wq[j][r], we[j][r], wd[j][r]);
            CHECK(o.q[0][count] == 0xC0FFEEu && o.p[0][count] == 0xC0FFEEu && o.d[0][count] == 0x5A, "wrote behind count");
            if (!second) CHECK(o.untouched(1), "the second triple was written through NULL-ness");
            ++*cases;
        }
    // an invalid byte inside the last read with a window: its buffer index, outputs untouched
    for (size_t r = count; r-- > 0;) {
        if (lens[r] < k) continue;
        const size_t at = (size_t)off[r] + lens[r] - 1;
        const uint8_t keep = ascii[at];
        ascii[at] = 'N';
        Six o(count);
        const long long bad = fixed ? bitnuc_host::reads_edist_best_small(ascii, lens[0], count, k, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1])
                                    : bitnuc_host::reads_edist_best_batch_small(ascii, off.data(), count, k, queries, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]);
        CHECK(bad == (long long)at && o.untouched(0), "k %zu: invalid byte at %zu reported as %lld", k, at, bad);
        ascii[at] = keep;
        ++*cases;
        break;
    }
    UNPOISON(buf, gap + total + 1);
    UNPOISON(words, (nwords + 1) * 8);
    free(buf);
    free(words);
}

int main() {
    unsigned long long cases = 0;
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    for (size_t k : ks) {
        const std::vector<size_t> lens = {150, k - 1, 64, 0, k, 63, k + 1, 65, 127, k - 1, 128, 129, 257, 0};
        for (size_t nq : {(size_t)1, (size_t)2, (size_t)5}) {
            std::vector<uint64_t> queries(nq);
            std::vector<PatternSets> patterns(nq);
            for (size_t q = 0; q < nq; ++q) {
                queries[q] = next_u64(); // junk above 2k
                for (int c = 0; c < 4; ++c) patterns[q].allow[c] = (uint32_t)next_u64() | (uint32_t)next_u64(); // dense sets, junk above k
            }
            run(k, lens, queries.data(), nq, false, &cases);
            run(k, lens, patterns.data(), nq, false, &cases);
            for (size_t n : {k, (size_t)64, (size_t)65, (size_t)150}) {
                run(k, std::vector<size_t>(3, n), queries.data(), nq, true, &cases);
                run(k, std::vector<size_t>(3, n), patterns.data(), nq, true, &cases);
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads edist best host ok: %llu cases\n", cases);
    return 0;
}
