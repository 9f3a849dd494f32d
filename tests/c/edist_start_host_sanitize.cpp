// The host side of the indel-tolerant family's second stage (bitnuc_amd/csrc/edist_start_host.h: reads_edist_start_small, reads_edist_start_batch_small,
// kmer_edist_start_small; the backward bit-parallel walk) under AddressSanitizer + UndefinedBehaviorSanitizer, against the definition: one plain Levenshtein
// table (D[0][j] = j, D[i][0] = i) per candidate substring t[s, e), s in [e - w, e], w = min(e - a, 2k - 1), and the lexicographic minimum of (distance,
// length).  k in {1, 2, 15, 16, 17, 31, 32}, exact queries and patterns (one of them with an empty set), the three geometries, both anchors, ASCII and
// packed.  Exactly sized heap buffers; in the ASCII buffers EVERY byte outside the walked ranges of the live items is 'N' and poisoned: the host form
// neither validates nor reads it.  Skipped items (query >= nq, query = UINT32_MAX, end > len, end < floor, 0xA5A5A5A5) write fills.  An invalid byte planted
// in a walked range: its buffer index, outputs untouched.  dist as a NULL pointer: start unchanged.
#include "../../bitnuc_amd/csrc/edist_start_host.h"

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

// the Levenshtein distance of the pattern's k positions to the n codes at t
static uint32_t lev(const uint8_t *t, size_t n, size_t k, const PatternSets &p) {
    std::vector<uint32_t> prev(n + 1), cur(n + 1);
    for (size_t j = 0; j <= n; ++j) prev[j] = (uint32_t)j;
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
    return prev[n];
}

// the definition; codes: the item's text
static void ref_start(const uint8_t *codes, uint64_t a, uint64_t e, size_t k, const PatternSets &p, uint64_t *start, uint8_t *dist) {
    const uint64_t w = e - a < 2 * k - 1 ? e - a : 2 * k - 1;
    uint32_t best = ~0u;
    uint64_t best_len = 0;
    for (uint64_t c = 0; c <= w; ++c) { // ascending lengths: the first minimum is the shortest
        const uint32_t d = lev(codes + e - c, (size_t)c, k, p);
        if (d < best) best = d, best_len = c;
    }
    *start = e - best_len;
    *dist = (uint8_t)best;
}

struct Batch {
    std::vector<uint64_t> off;  // count + 1
    std::vector<uint8_t> codes; // all reads back to back
};

static const char LUT[] = "ACGTacgt";

static void run(size_t k, bool ragged, int from_end, size_t pos, bool patterns) {
    const size_t count = 40, nq = 3;
    Batch b;
    b.off.push_back(0);
    const size_t fixed_len = 2 * k + 11;
    for (size_t r = 0; r < count; ++r) {
        const size_t len = ragged ? (size_t)(next_u64() % (3 * k + 20)) : fixed_len;
        b.off.push_back(b.off.back() + len);
    }
    b.codes.resize((size_t)b.off.back());
    for (auto &c : b.codes) c = (uint8_t)(next_u64() & 3);
    std::vector<uint64_t> qw(nq);
    std::vector<PatternSets> ps(nq);
    for (size_t q = 0; q < nq; ++q) {
        qw[q] = next_u64();
        ps[q] = bitnuc_host::pattern_of_2bit(qw[q], k);
        if (patterns) {
            for (int c = 0; c < 4; ++c) ps[q].allow[c] |= (uint32_t)next_u64() & (uint32_t)next_u64(); // wider sets
            if (q == 1) for (int c = 0; c < 4; ++c) ps[q].allow[c] &= ~1u;                              // position 0: the empty set
        }
    }
    // plant copies of query 0 so that small distances occur
    for (size_t r = 0; r < count; r += 2) {
        const size_t len = (size_t)(b.off[r + 1] - b.off[r]);
        if (len < k) continue;
        const size_t at = (size_t)b.off[r] + (size_t)(next_u64() % (len - k + 1));
        for (size_t i = 0; i < k; ++i) b.codes[at + i] = (uint8_t)((qw[0] >> (2 * i)) & 3);
    }
    std::vector<uint32_t> query(count), end(count);
    std::vector<uint64_t> want_start(count);
    std::vector<uint8_t> want_dist(count);
    // exactly sized buffers; ASCII: 'N' everywhere but in the walked ranges
    uint8_t *ascii = (uint8_t *)malloc(b.codes.size() ? b.codes.size() : 1);
    memset(ascii, 'N', b.codes.size());
    std::vector<char> walked(b.codes.size(), 0);
    for (size_t r = 0; r < count; ++r) {
        const uint64_t len = b.off[r + 1] - b.off[r];
        const uint64_t a = bitnuc_host::edist_start_floor(len, k, from_end, pos);
        query[r] = (uint32_t)(next_u64() % nq);
        end[r] = (uint32_t)(a <= len ? a + next_u64() % (len - a + 1) : 0);
        switch (r % 10) { // skipped items
        case 3: query[r] = (uint32_t)nq; break;
        case 5: query[r] = 0xFFFFFFFFu; break;
        case 7: end[r] = (uint32_t)len + 1; break;
        case 8: end[r] = r % 20 == 8 ? 0xA5A5A5A5u : (a ? (uint32_t)a - 1 : (uint32_t)len + 2); break;
        default: break;
        }
        const bool live = query[r] < nq && end[r] <= len && end[r] >= a;
        want_start[r] = 0xFFFFFFFFu, want_dist[r] = 0xFF;
        if (!live) continue;
        ref_start(b.codes.data() + b.off[r], a, end[r], k, ps[query[r]], &want_start[r], &want_dist[r]);
        const uint64_t w = end[r] - a < 2 * k - 1 ? end[r] - a : 2 * k - 1;
        for (uint64_t i = end[r] - w; i < end[r]; ++i) walked[(size_t)(b.off[r] + i)] = 1;
    }
    for (size_t i = 0; i < b.codes.size(); ++i)
        if (walked[i]) ascii[i] = (uint8_t)LUT[b.codes[i] + 4 * (next_u64() & 1)];
    for (size_t i = 0; i < b.codes.size(); ++i)
        if (!walked[i]) POISON(ascii + i, 1);
    // packed: per read ceil(len / 32) words, junk in the pad bits
    std::vector<uint64_t> woff(count + 1, 0);
    for (size_t r = 0; r < count; ++r) woff[r + 1] = woff[r] + (b.off[r + 1] - b.off[r] + 31) / 32;
    uint64_t *words = (uint64_t *)malloc(woff[count] ? (size_t)woff[count] * 8 : 8);
    for (size_t i = 0; i < woff[count]; ++i) words[i] = next_u64();
    for (size_t r = 0; r < count; ++r)
        for (uint64_t j = 0; j < b.off[r + 1] - b.off[r]; ++j) {
            uint64_t &wd = words[woff[r] + j / 32];
            wd = (wd & ~(3ull << (2 * (j % 32)))) | ((uint64_t)b.codes[(size_t)(b.off[r] + j)] << (2 * (j % 32)));
        }
    uint32_t *start = (uint32_t *)malloc(count * 4);
    uint8_t *dist = (uint8_t *)malloc(count);
    for (int packed = 0; packed < 2; ++packed) {
        for (int with_dist = 1; with_dist >= 0; --with_dist) {
            memset(start, 0x5A, count * 4);
            memset(dist, 0x5A, count);
            long long bad;
            uint8_t *dp = with_dist ? dist : nullptr;
#define CALL(Q)                                                                                                                                              \
    (ragged ? (packed ? bitnuc_host::reads_edist_start_batch_small<true>(words, woff.data(), b.off.data(), count, k, from_end, pos, Q, nq, query.data(),     \
                                                                        end.data(), start, dp)                                                               \
                      : bitnuc_host::reads_edist_start_batch_small<false>(ascii, nullptr, b.off.data(), count, k, from_end, pos, Q, nq, query.data(),        \
                                                                         end.data(), start, dp))                                                             \
            : (packed ? bitnuc_host::reads_edist_start_small<true>(words, fixed_len, count, k, from_end, pos, Q, nq, query.data(), end.data(), start, dp)    \
                      : bitnuc_host::reads_edist_start_small<false>(ascii, fixed_len, count, k, from_end, pos, Q, nq, query.data(), end.data(), start, dp)))
            bad = patterns ? CALL(ps.data()) : CALL(qw.data());
            CHECK(bad == -1, "k %zu: invalid byte %lld reported in a clean batch", k, bad);
            for (size_t r = 0; r < count; ++r) {
                CHECK(start[r] == (uint32_t)want_start[r], "k %zu ragged %d end-anchor %d pos %zu packed %d patterns %d read %zu: start %u, want %u", k, ragged, from_end,
                      pos, packed, patterns, r, start[r], (uint32_t)want_start[r]);
                CHECK(dist[r] == (with_dist ? want_dist[r] : 0x5A), "k %zu read %zu: dist %u, want %u", k, r, dist[r], want_dist[r]);
            }
        }
    }
    // an invalid byte in a walked range: its index, outputs untouched
    for (size_t i = 0; i < b.codes.size(); ++i) {
        if (!walked[i]) continue;
        const uint8_t keep = ascii[i];
        ascii[i] = 'N';
        memset(start, 0x5A, count * 4);
        memset(dist, 0x5A, count);
        uint8_t *dp = dist;
        const int packed = 0;
        const long long bad = patterns ? CALL(ps.data()) : CALL(qw.data());
        CHECK(bad == (long long)i, "k %zu: invalid byte at %zu reported as %lld", k, i, bad);
        for (size_t r = 0; r < count; ++r) CHECK(start[r] == 0x5A5A5A5Au && dist[r] == 0x5A, "outputs written on an invalid byte");
        ascii[i] = keep;
        i += 37; // a few positions per batch
    }
#undef CALL
    // along a reference: the whole batch as one text, the floor 0
    {
        const size_t n = b.codes.size(), m = 25;
        std::vector<uint64_t> e64(m), s64(m);
        std::vector<uint32_t> qi(m);
        std::vector<uint8_t> d8(m);
        UNPOISON(ascii, n ? n : 1);
        for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)LUT[b.codes[i]];
        for (size_t i = 0; i < m; ++i) e64[i] = i == 3 ? n + 1 : i == 4 ? 0xA5A5A5A5A5A5A5A5ull : next_u64() % (n + 1), qi[i] = i == 5 ? (uint32_t)nq : (uint32_t)(next_u64() % nq);
        uint64_t *wref = (uint64_t *)malloc(((n + 31) / 32 + 1) * 8);
        for (size_t i = 0; i < (n + 31) / 32; ++i) wref[i] = next_u64();
        for (size_t j = 0; j < n; ++j) wref[j / 32] = (wref[j / 32] & ~(3ull << (2 * (j % 32)))) | ((uint64_t)b.codes[j] << (2 * (j % 32)));
        for (int packed = 0; packed < 2; ++packed) {
            for (int indexed = 0; indexed < 2; ++indexed) {
                const uint32_t *qp = indexed ? qi.data() : nullptr;
                long long bad;
                if (patterns) bad = packed ? bitnuc_host::kmer_edist_start_small<true>(wref, n, k, ps.data(), nq, qp, e64.data(), m, s64.data(), d8.data())
                                           : bitnuc_host::kmer_edist_start_small<false>(ascii, n, k, ps.data(), nq, qp, e64.data(), m, s64.data(), d8.data());
                else bad = packed ? bitnuc_host::kmer_edist_start_small<true>(wref, n, k, qw.data(), nq, qp, e64.data(), m, s64.data(), d8.data())
                                  : bitnuc_host::kmer_edist_start_small<false>(ascii, n, k, qw.data(), nq, qp, e64.data(), m, s64.data(), d8.data());
                CHECK(bad == -1, "reference: invalid byte %lld", bad);
                for (size_t i = 0; i < m; ++i) {
                    const uint32_t q = indexed ? qi[i] : 0;
                    uint64_t ws = ~0ull;
                    uint8_t wd = 0xFF;
                    if (q < nq && e64[i] <= n) ref_start(b.codes.data(), 0, e64[i], k, ps[q], &ws, &wd);
                    CHECK(s64[i] == ws && d8[i] == wd, "reference k %zu packed %d item %zu: (%llu, %u), want (%llu, %u)", k, packed, i, (unsigned long long)s64[i], d8[i],
                          (unsigned long long)ws, wd);
                }
            }
        }
        free(wref);
    }
    free(start);
    free(dist);
    free(words);
    free(ascii);
}

int main() {
    const size_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    for (size_t k : ks)
        for (int ragged = 0; ragged < 2; ++ragged)
            for (int from_end = 0; from_end < 2; ++from_end)
                for (size_t pos : {(size_t)0, (size_t)3})
                    for (int patterns = 0; patterns < 2; ++patterns) run(k, ragged != 0, from_end, pos, patterns != 0);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("edist start host ok\n");
    return 0;
}
