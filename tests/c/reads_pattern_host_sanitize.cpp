// The host forms of the per-read matchers with PATTERN queries (PatternSets: a set of bases per position) -- the templates of reads_best_host.h,
// reads_best2_host.h, reads_batch_host.h, reads_anchored_host.h and reads_anchored_batch_host.h instantiated with the other query kind -- under
// AddressSanitizer + UndefinedBehaviorSanitizer, against a brute force written from the definition: pdist = #{ i < k : base i not in S_i }, per read and
// pattern the minimum over the admissible offsets and its leftmost window, the best the first minimum over the patterns, the runner-up the first minimum
// over the OTHER patterns.  k in {1, 16, 31, 32}; 1 / 2 / 3 / 17 patterns of random sets (empty and N positions, an all-N and an all-empty pattern, two equal
// ones), junk allow bits at positions >= k; fixed-length and ragged batches, ASCII (either case) and packed (junk pad bits), on exactly sized heap
// buffers: a read or write one element outside is the sanitizer's finding.
#include "../../bitnuc_amd/csrc/reads_best_host.h"
#include "../../bitnuc_amd/csrc/reads_best2_host.h"
#include "../../bitnuc_amd/csrc/reads_batch_host.h"
#include "../../bitnuc_amd/csrc/reads_anchored_host.h"
#include "../../bitnuc_amd/csrc/reads_anchored_batch_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using bitnuc_host::PatternSets;

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

static uint32_t ref_pdist(const uint8_t *codes, size_t k, const PatternSets &p) {
    uint32_t d = 0;
    for (size_t i = 0; i < k; ++i) d += !((p.allow[codes[i]] >> i) & 1u);
    return d;
}

// exactly sized outputs: `triples` x (query, pos, dist)
struct Outs {
    uint32_t *q[2], *p[2];
    uint8_t *d[2];
    explicit Outs(size_t count) {
        for (int j = 0; j < 2; ++j) {
            q[j] = (uint32_t *)malloc(count ? count * 4 : 1), p[j] = (uint32_t *)malloc(count ? count * 4 : 1), d[j] = (uint8_t *)malloc(count ? count : 1);
            for (size_t r = 0; r < count; ++r) q[j][r] = p[j][r] = 0x11111111u, d[j][r] = 0x11;
        }
    }
    ~Outs() {
        for (int j = 0; j < 2; ++j) free(q[j]), free(p[j]), free(d[j]);
    }
};

struct Want {
    std::vector<uint32_t> q[2], p[2], d[2];
};

// the brute force: read r's admissible offsets are first[r] .. first[r] + num[r] - 1 from code starts[r]
static Want brute(const std::vector<uint8_t> &codes, const std::vector<size_t> &starts, const std::vector<size_t> &first, const std::vector<size_t> &num, size_t k,
                  const PatternSets *pats, size_t nq) {
    const size_t count = starts.size();
    Want w;
    for (int j = 0; j < 2; ++j) w.q[j].assign(count, 0xFFFFFFFFu), w.p[j].assign(count, 0xFFFFFFFFu), w.d[j].assign(count, 0xFF);
    std::vector<uint32_t> md(nq), mi(nq);
    for (size_t r = 0; r < count; ++r) {
        if (!num[r] || !nq) continue;
        for (size_t q = 0; q < nq; ++q) {
            md[q] = 0xFF;
            for (size_t i = first[r]; i < first[r] + num[r]; ++i) {
                const uint32_t d = ref_pdist(codes.data() + starts[r] + i, k, pats[q]);
                if (d < md[q]) md[q] = d, mi[q] = (uint32_t)i;
            }
        }
        for (int j = 0; j < 2; ++j)
            for (size_t q = 0; q < nq; ++q)
                if ((j == 0 || q != w.q[0][r]) && md[q] < w.d[j][r]) w.d[j][r] = md[q], w.q[j][r] = (uint32_t)q, w.p[j][r] = mi[q];
    }
    return w;
}

static void compare(const char *what, const Outs &o, const Want &w, size_t count, int triples, size_t k, size_t nq) {
    for (int j = 0; j < triples; ++j)
        for (size_t r = 0; r < count; ++r)
            CHECK(o.q[j][r] == w.q[j][r] && o.p[j][r] == w.p[j][r] && o.d[j][r] == w.d[j][r], "%s rank %d k %zu nq %zu read %zu: (%u, %u, %u) vs (%u, %u, %u)", what, j, k,
                  nq, r, o.q[j][r], o.p[j][r], (unsigned)o.d[j][r], w.q[j][r], w.p[j][r], w.d[j][r]);
}

static PatternSets random_pattern(size_t k) {
    PatternSets p = {{0u, 0u, 0u, 0u}};
    for (size_t i = 0; i < k; ++i) {
        const unsigned r = (unsigned)(next_u64() & 7);
        const unsigned set = r == 0 ? 0u : r == 1 ? 0xFu : (unsigned)(next_u64() & 0xF);
        for (unsigned c = 0; c < 4; ++c) p.allow[c] |= ((set >> c) & 1u) << i;
    }
    if (k < 32)
        for (unsigned c = 0; c < 4; ++c) p.allow[c] |= (uint32_t)next_u64() << k; // junk at positions >= k: ignored
    return p;
}

int main() {
    const size_t ks[] = {1, 16, 31, 32};
    const size_t nqs[] = {1, 2, 3, 17};
    unsigned long long cases = 0;
    for (size_t k : ks)
        for (size_t nq : nqs) {
            PatternSets *pats = (PatternSets *)malloc(nq * sizeof(PatternSets));
            for (size_t q = 0; q < nq; ++q) pats[q] = random_pattern(k);
            if (nq == 17) {
                const uint32_t ones = k == 32 ? ~0u : (1u << k) - 1u;
                pats[4] = PatternSets{{ones, ones, ones, ones}}; // all-N: distance 0 everywhere
                pats[9] = PatternSets{{0u, 0u, 0u, 0u}};         // all-empty: distance k everywhere
                pats[12] = pats[4];                              // an equal pattern: the runner-up of its twin
            }
            if (nq == 3) pats[2] = pats[0];

            // ---- a fixed-length batch ----
            for (size_t read_len : {k, k + 5, (size_t)70}) {
                const size_t count = 9, wpr = (read_len + 31) / 32, n = count * read_len;
                std::vector<uint8_t> codes(n);
                for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                uint8_t *ascii = (uint8_t *)malloc(n);
                for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
                uint64_t *words = (uint64_t *)malloc(count * wpr * 8);
                memset(words, 0, count * wpr * 8);
                for (size_t r = 0; r < count; ++r) {
                    for (size_t i = 0; i < read_len; ++i) words[r * wpr + i / 32] |= (uint64_t)codes[r * read_len + i] << (2 * (i % 32));
                    if (read_len % 32) words[r * wpr + wpr - 1] |= next_u64() & ~((1ull << (2 * (read_len % 32))) - 1);
                }
                std::vector<size_t> starts(count), first(count, 0), num(count, read_len - k + 1);
                for (size_t r = 0; r < count; ++r) starts[r] = r * read_len;
                const Want whole = brute(codes, starts, first, num, k, pats, nq);
                {
                    Outs o(count);
                    CHECK(bitnuc_host::reads_hdist_best_small(ascii, read_len, count, k, pats, nq, o.q[0], o.p[0], o.d[0]) == -1, "best: bad byte");
                    compare("best", o, whole, count, 1, k, nq);
                    Outs o2(count);
                    bitnuc_host::reads_hdist_best_packed_small(words, read_len, count, k, pats, nq, o2.q[0], o2.p[0], o2.d[0]);
                    compare("best packed", o2, whole, count, 1, k, nq);
                }
                {
                    Outs o(count);
                    CHECK(bitnuc_host::reads_hdist_best2_small(ascii, read_len, count, k, pats, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]) == -1, "best2: bad byte");
                    compare("best2", o, whole, count, 2, k, nq);
                    Outs o2(count);
                    bitnuc_host::reads_hdist_best2_packed_small(words, read_len, count, k, pats, nq, o2.q[0], o2.p[0], o2.d[0], o2.q[1], o2.p[1], o2.d[1]);
                    compare("best2 packed", o2, whole, count, 2, k, nq);
                }
                const size_t last = read_len - k;
                for (size_t lo : {(size_t)0, last / 2, last}) {
                    const size_t width = last - lo + 1 < 4 ? last - lo + 1 : 4; // up to four offsets from lo
                    std::vector<size_t> f(count, lo), m(count, width);
                    const Want part = brute(codes, starts, f, m, k, pats, nq);
                    for (int second = 1; second >= 0; --second) {
                        Outs o(count);
                        CHECK(bitnuc_host::reads_hdist_anchored_small(ascii, read_len, count, k, lo, width, pats, nq, o.q[0], o.p[0], o.d[0], second ? o.q[1] : nullptr,
                                                                      second ? o.p[1] : nullptr, second ? o.d[1] : nullptr) == -1,
                              "anchored: bad byte");
                        compare("anchored", o, part, count, 1 + second, k, nq);
                        Outs o2(count);
                        bitnuc_host::reads_hdist_anchored_packed_small(words, read_len, count, k, lo, width, pats, nq, o2.q[0], o2.p[0], o2.d[0], second ? o2.q[1] : nullptr,
                                                                       second ? o2.p[1] : nullptr, second ? o2.d[1] : nullptr);
                        compare("anchored packed", o2, part, count, 1 + second, k, nq);
                        ++cases;
                    }
                }
                // an N in a read is an invalid base whatever the patterns allow: its index, the outputs untouched
                const size_t at = (size_t)(next_u64() % n);
                const uint8_t keep = ascii[at];
                ascii[at] = 'N';
                Outs o(count);
                CHECK(bitnuc_host::reads_hdist_best2_small(ascii, read_len, count, k, pats, nq, o.q[0], o.p[0], o.d[0], o.q[1], o.p[1], o.d[1]) == (long long)at, "N at %zu", at);
                for (size_t r = 0; r < count; ++r) CHECK(o.q[0][r] == 0x11111111u && o.d[1][r] == 0x11, "outputs written on an invalid byte");
                ascii[at] = keep;
                free(ascii);
                free(words);
                ++cases;
            }

            // ---- a ragged batch ----
            for (int from_end = 0; from_end < 2; ++from_end)
                for (size_t lo : {(size_t)0, (size_t)3}) {
                    const size_t width = 4, hi = lo + width - 1;
                    std::vector<size_t> lens = {0, k - 1, k, k + lo, k + lo + 2, k + lo + width, 150, 0, 77};
                    if (k > 2) lens.push_back(k / 2);
                    const size_t count = lens.size();
                    std::vector<uint64_t> off(count + 1, 0), woff(count + 1, 0);
                    for (size_t r = 0; r < count; ++r) off[r + 1] = off[r] + lens[r], woff[r + 1] = woff[r] + (lens[r] + 31) / 32;
                    const size_t n = (size_t)off[count], nw = (size_t)woff[count];
                    std::vector<uint8_t> codes(n);
                    for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)(next_u64() & 3);
                    uint8_t *ascii = (uint8_t *)malloc(n);
                    for (size_t i = 0; i < n; ++i) ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((next_u64() & 1) ? 0x20 : 0));
                    uint64_t *words = (uint64_t *)malloc(nw * 8);
                    memset(words, 0, nw * 8);
                    for (size_t r = 0; r < count; ++r) {
                        uint64_t *w = words + woff[r];
                        for (size_t i = 0; i < lens[r]; ++i) w[i / 32] |= (uint64_t)codes[off[r] + i] << (2 * (i % 32));
                        if (lens[r] % 32) w[(lens[r] - 1) / 32] |= next_u64() & ~((1ull << (2 * (lens[r] % 32))) - 1);
                    }
                    std::vector<size_t> starts(count), first(count, 0), num(count, 0), f0(count, 0), all(count, 0);
                    for (size_t r = 0; r < count; ++r) {
                        starts[r] = (size_t)off[r];
                        if (lens[r] < k) continue;
                        const size_t last = lens[r] - k;
                        all[r] = last + 1;
                        for (size_t i = 0; i <= last; ++i) {
                            const size_t key = from_end ? last - i : i;
                            if (key < lo || key > hi) continue;
                            if (!num[r]) first[r] = i;
                            ++num[r];
                        }
                    }
                    const Want whole = brute(codes, starts, f0, all, k, pats, nq), part = brute(codes, starts, first, num, k, pats, nq);
                    {
                        Outs o(count);
                        CHECK(bitnuc_host::reads_hdist_best_batch_small(ascii, off.data(), count, k, pats, nq, o.q[0], o.p[0], o.d[0]) == -1, "best_batch: bad byte");
                        compare("best_batch", o, whole, count, 1, k, nq);
                        Outs o2(count);
                        bitnuc_host::reads_hdist_best_batch_packed_small(words, woff.data(), off.data(), count, k, pats, nq, o2.q[0], o2.p[0], o2.d[0]);
                        compare("best_batch packed", o2, whole, count, 1, k, nq);
                    }
                    for (int second = 1; second >= 0; --second) {
                        Outs o(count);
                        CHECK(bitnuc_host::reads_hdist_anchored_batch_small(ascii, off.data(), count, k, from_end, lo, hi, pats, nq, o.q[0], o.p[0], o.d[0],
                                                                            second ? o.q[1] : nullptr, second ? o.p[1] : nullptr, second ? o.d[1] : nullptr) == -1,
                              "anchored_batch: bad byte");
                        compare("anchored_batch", o, part, count, 1 + second, k, nq);
                        Outs o2(count);
                        bitnuc_host::reads_hdist_anchored_batch_packed_small(words, woff.data(), off.data(), count, k, from_end, lo, hi, pats, nq, o2.q[0], o2.p[0], o2.d[0],
                                                                             second ? o2.q[1] : nullptr, second ? o2.p[1] : nullptr, second ? o2.d[1] : nullptr);
                        compare("anchored_batch packed", o2, part, count, 1 + second, k, nq);
                        ++cases;
                    }
                    free(ascii);
                    free(words);
                }
            free(pats);
        }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("reads pattern host ok: %llu cases\n", cases);
    return 0;
}
