// The host 3' adapter per read (bitnuc_amd/csrc/reads_edist_adapter_host.h: reads_edist_adapter_small / _packed_small / _batch_small /
// _batch_packed_small) under AddressSanitizer + UndefinedBehaviorSanitizer, against the plain dynamic programme over ALL rows: D[0][j] = 0, D[i][0] = i,
// D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1); the full candidates (i = k, any j) and the overhang candidates (min_overlap <= i < k,
// j = n) within floor(i num / den), the smallest (misses, d, query, j); the cut as a Levenshtein minimum over the starts, one plain DP per start.
// k in {1, 2, 15, 16, 17, 31, 32}, reads of k - 1, k, k + 1, 0, 63, 64, 65, 127, 128, 129 and 150 bases, 1 / 2 / 5 queries, exact queries and patterns, both
// layouts, rates 0/1, 1/10, 1/5, 1/1, min_overlap 1, 3 (where k allows) and k.  Exactly sized heap buffers.  Ragged: the reads lie behind a gap of 'N' bytes,
// and EVERY byte outside the reads of at least k bases is poisoned: the host form neither validates nor reads it; the packed words are exactly sized, the
// words of reads shorter than k are poisoned, the pad bits hold junk.  An invalid byte planted inside a read: its buffer index, outputs untouched.
#include "../../bitnuc_amd/csrc/reads_edist_adapter_host.h"

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

static PatternSets sets_of(const PatternSets &p, size_t) { return p; }
static PatternSets sets_of(uint64_t q, size_t k) { return bitnuc_host::pattern_of_2bit(q, k); }

// the plain DP over all rows of the first `rows` positions against t[0, n): D as (rows + 1) x (n + 1); anchored: D[0][j] = j instead of 0
static std::vector<std::vector<uint32_t>> plain_dp(const uint8_t *t, size_t n, size_t rows, const PatternSets &p, bool anchored) {
    std::vector<std::vector<uint32_t>> D(rows + 1, std::vector<uint32_t>(n + 1, 0));
    for (size_t j = 0; j <= n; ++j) D[0][j] = anchored ? (uint32_t)j : 0u;
    for (size_t i = 1; i <= rows; ++i) {
        D[i][0] = (uint32_t)i;
        for (size_t j = 1; j <= n; ++j) {
            uint32_t v = D[i - 1][j - 1] + (((p.allow[t[j - 1]] >> (i - 1)) & 1u) ? 0u : 1u);
            if (D[i - 1][j] + 1 < v) v = D[i - 1][j] + 1;
            if (D[i][j - 1] + 1 < v) v = D[i][j - 1] + 1;
            D[i][j] = v;
        }
    }
    return D;
}

struct Five { uint32_t adapter, cut, end; uint8_t overlap, dist; };

template <class Q>
static Five ref_read(const uint8_t *t, size_t n, size_t k, const Q *queries, size_t nq, size_t min_overlap, size_t num, size_t den) {
    Five f{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFF, 0xFF};
    if (n < k) return f;
    uint64_t best[4] = {~0ull, 0, 0, 0}; // misses, d, q, j
    size_t best_i = 0;
    const auto take = [&](uint64_t misses, uint64_t d, uint64_t q, uint64_t j, size_t i) {
        const uint64_t c[4] = {misses, d, q, j};
        for (int x = 0; x < 4; ++x) {
            if (c[x] < best[x]) break;
            if (c[x] > best[x]) return;
            if (x == 3) return;
        }
        memcpy(best, c, sizeof c);
        best_i = i;
    };
    for (size_t q = 0; q < nq; ++q) {
        const auto D = plain_dp(t, n, k, sets_of(queries[q], k), false);
        for (size_t j = 1; j <= n; ++j)
            if (D[k][j] <= k * num / den) take(D[k][j], D[k][j], q, j, k);
        for (size_t i = min_overlap; i < k; ++i)
            if (D[i][n] <= i * num / den) take(k - i + D[i][n], D[i][n], q, n, i);
    }
    if (best[0] == ~0ull) return f;
    const size_t e = (size_t)best[3], i = best_i, w = e < 2 * i - 1 ? e : 2 * i - 1;
    uint32_t low = ~0u;
    size_t at = e;
    for (size_t s = e;; --s) { // the shortest substring first: ties keep it
        const auto D = plain_dp(t + s, e - s, i, sets_of(queries[best[2]], k), true);
        if (D[i][e - s] < low) low = D[i][e - s], at = s;
        if (s == e - w) break;
    }
    CHECK(low == best[1], "the cut's distance %u is not the candidate's %u", low, (unsigned)best[1]);
    return Five{(uint32_t)best[2], (uint32_t)at, (uint32_t)e, (uint8_t)i, (uint8_t)best[1]};
}

static const char kBases[] = "ACGTacgt";

template <class Q> static Q make_query(size_t k);
template <> uint64_t make_query<uint64_t>(size_t) { return next_u64(); }
template <> PatternSets make_query<PatternSets>(size_t k) {
    PatternSets p{};
    for (size_t i = 0; i < k; ++i) {
        const unsigned set = next_u64() % 8 == 0 ? (unsigned)(next_u64() % 16) : 1u << (next_u64() % 4);
        for (unsigned c = 0; c < 4; ++c)
            if ((set >> c) & 1u) p.allow[c] |= 1u << i;
    }
    return p;
}

template <class Q>
static void run_case(size_t k, const std::vector<size_t> &lens, size_t nq, size_t min_overlap, size_t num, size_t den) {
    using namespace bitnuc_host;
    const size_t count = lens.size();
    std::vector<Q> queries(nq);
    for (auto &q : queries) q = make_query<Q>(k);
    const AdapterRule rule = adapter_rule(min_overlap, num, den);
    const size_t gap = 5;
    std::vector<uint64_t> off(count + 1), woff(count + 1);
    off[0] = gap, woff[0] = 0;
    for (size_t r = 0; r < count; ++r) off[r + 1] = off[r] + lens[r], woff[r + 1] = woff[r] + (lens[r] + 31) / 32;
    const size_t total = (size_t)off[count];
    uint8_t *seq = (uint8_t *)malloc(total ? total : 1);
    memset(seq, 'N', total);
    std::vector<std::vector<uint8_t>> codes(count);
    for (size_t r = 0; r < count; ++r) {
        codes[r].resize(lens[r]);
        for (size_t j = 0; j < lens[r]; ++j) {
            const unsigned pick = (unsigned)(next_u64() % 8);
            seq[off[r] + j] = (uint8_t)kBases[pick];
            codes[r][j] = (uint8_t)(pick & 3);
        }
        // half of the reads end with a prefix of a query, some with one substitution
        if (lens[r] >= k && next_u64() % 2) {
            const PatternSets p = sets_of(queries[next_u64() % nq], k);
            const size_t i = 1 + (size_t)(next_u64() % k);
            for (size_t a = 0; a < i; ++a) {
                unsigned c = 0;
                while (c < 3 && !((p.allow[c] >> a) & 1u)) ++c;
                if (i > 4 && a == i / 2 && next_u64() % 2) c = (c + 1) & 3;
                seq[off[r] + lens[r] - i + a] = (uint8_t)kBases[c];
                codes[r][lens[r] - i + a] = (uint8_t)c;
            }
        }
    }
    const size_t nwords = (size_t)woff[count];
    uint64_t *words = (uint64_t *)malloc(nwords ? nwords * 8 : 8);
    for (size_t r = 0; r < count; ++r)
        for (size_t w = 0; w < (lens[r] + 31) / 32; ++w) {
            uint64_t x = next_u64(); // junk in the pad bits
            for (size_t b = 0; b < 32 && 32 * w + b < lens[r]; ++b) x = (x & ~(3ull << (2 * b))) | ((uint64_t)codes[r][32 * w + b] << (2 * b));
            words[woff[r] + w] = x;
        }
    std::vector<Five> want(count);
    for (size_t r = 0; r < count; ++r) want[r] = ref_read(codes[r].data(), lens[r], k, queries.data(), nq, min_overlap, num, den);
    POISON(seq, gap);
    for (size_t r = 0; r < count; ++r)
        if (lens[r] < k) {
            POISON(seq + off[r], lens[r]);
            POISON(words + woff[r], 8 * (size_t)(woff[r + 1] - woff[r]));
        }
    uint32_t *adapter = (uint32_t *)malloc(4 * count), *cut = (uint32_t *)malloc(4 * count), *end = (uint32_t *)malloc(4 * count);
    uint8_t *overlap = (uint8_t *)malloc(count), *dist = (uint8_t *)malloc(count);
    const auto same = [&](const char *what) {
        for (size_t r = 0; r < count; ++r)
            CHECK(adapter[r] == want[r].adapter && cut[r] == want[r].cut && end[r] == want[r].end && overlap[r] == want[r].overlap && dist[r] == want[r].dist,
                  "%s k=%zu len=%zu nq=%zu mo=%zu %zu/%zu read %zu: (%u %u %u %u %u) want (%u %u %u %u %u)", what, k, lens[r], nq, min_overlap, num, den, r, adapter[r],
                  cut[r], end[r], overlap[r], dist[r], want[r].adapter, want[r].cut, want[r].end, want[r].overlap, want[r].dist);
    };
    const auto reset = [&]() { memset(adapter, 0x5A, 4 * count), memset(cut, 0x5A, 4 * count), memset(end, 0x5A, 4 * count), memset(overlap, 0x5A, count), memset(dist, 0x5A, count); };
    reset();
    CHECK(reads_edist_adapter_batch_small(seq, off.data(), count, k, queries.data(), nq, rule, adapter, cut, end, overlap, dist) == -1, "ragged: reported invalid");
    same("ragged ascii");
    reset();
    reads_edist_adapter_batch_packed_small(words, woff.data(), off.data(), count, k, queries.data(), nq, rule, adapter, cut, end, overlap, dist);
    same("ragged packed");
    // an invalid byte in the last read of at least k bases: its index, outputs untouched
    for (size_t r = count; r-- > 0;) {
        if (lens[r] < k) continue;
        const size_t at = (size_t)off[r] + lens[r] / 2;
        const uint8_t keep = seq[at];
        seq[at] = 'N';
        reset();
        const long long bad = reads_edist_adapter_batch_small(seq, off.data(), count, k, queries.data(), nq, rule, adapter, cut, end, overlap, dist);
        CHECK(bad == (long long)at, "invalid byte at %zu reported as %lld", at, bad);
        CHECK(adapter[0] == 0x5A5A5A5Au && dist[count - 1] == 0x5A, "outputs written with an invalid byte");
        seq[at] = keep;
        break;
    }
    // the fixed forms on the reads of the first length that holds k bases
    for (size_t r = 0; r < count; ++r) {
        if (lens[r] < k) continue;
        const size_t n = lens[r], wpr = (n + 31) / 32;
        uint8_t *one = (uint8_t *)malloc(2 * n);
        uint64_t *w2 = (uint64_t *)malloc(2 * wpr * 8);
        memcpy(one, seq + off[r], n), memcpy(one + n, seq + off[r], n);
        memcpy(w2, words + woff[r], wpr * 8), memcpy(w2 + wpr, words + woff[r], wpr * 8);
        reset();
        uint32_t a2[2], c2[2], e2[2];
        uint8_t o2[2], d2[2];
        CHECK(reads_edist_adapter_small(one, n, 2, k, queries.data(), nq, rule, a2, c2, e2, o2, d2) == -1, "fixed: reported invalid");
        for (int x = 0; x < 2; ++x)
            CHECK(a2[x] == want[r].adapter && c2[x] == want[r].cut && e2[x] == want[r].end && o2[x] == want[r].overlap && d2[x] == want[r].dist, "fixed ascii k=%zu n=%zu", k, n);
        reads_edist_adapter_packed_small(w2, n, 2, k, queries.data(), nq, rule, a2, c2, e2, o2, d2);
        for (int x = 0; x < 2; ++x)
            CHECK(a2[x] == want[r].adapter && c2[x] == want[r].cut && e2[x] == want[r].end && o2[x] == want[r].overlap && d2[x] == want[r].dist, "fixed packed k=%zu n=%zu", k, n);
        free(one), free(w2);
        break;
    }
    UNPOISON(seq, total ? total : 1);
    UNPOISON(words, nwords ? nwords * 8 : 8);
    free(seq), free(words), free(adapter), free(cut), free(end), free(overlap), free(dist);
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    const size_t rates[][2] = {{0, 1}, {1, 10}, {1, 5}, {1, 1}};
    int cases = 0;
    for (size_t k : ks) {
        const std::vector<size_t> lens = {k - 1, k, k + 1, 0, 63, 64, 65, 127, 128, 129, 150};
        for (const auto &rate : rates)
            for (size_t mo : {(size_t)1, (size_t)3, k}) {
                if (mo > k) continue;
                const size_t nq = cases % 3 == 0 ? 1 : cases % 3 == 1 ? 2 : 5;
                run_case<uint64_t>(k, lens, nq, mo, rate[0], rate[1]);
                run_case<PatternSets>(k, lens, nq, mo, rate[0], rate[1]);
                cases += 2;
            }
    }
    // the allowance table: exact for numerators a product would overflow with
    const bitnuc_host::AdapterRule big = bitnuc_host::adapter_rule(1, ~(size_t)0 - 1, ~(size_t)0);
    CHECK(big.allowed[32] == 31 && big.allowed[1] == 0, "allowed() overflowed");
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
