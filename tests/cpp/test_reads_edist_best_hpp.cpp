// The eight whole-read indel-tolerant methods of include/bitnuc.hpp (reads_edist_best, reads_pattern_edist_best, their _batch and _packed forms) on small
// batches, against the plain dynamic programme over the whole read, written from the definition: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] +
// [no match], D[i-1][j] + 1, D[i][j-1] + 1), the smallest D[k][j] and its first j, the end counted from the read's start; a read shorter than k: the fill.
// Small batches run on the library's host path; the C++ layer is what is under test: the argument order, the sizes of the vectors it allocates, the error
// mapping.
#include "bitnuc.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace bitnuc;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static unsigned code_of(char b) {
    switch (b & 0xDF) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    default: return 3;
    }
}

struct Top2 {
    uint32_t q[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, e[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    uint8_t d[2] = {0xFF, 0xFF};
};

// read [start, start + n) of s against every pattern, over its whole length
static Top2 brute(const std::string &s, size_t start, size_t n, size_t k, const std::vector<bitnuc_pattern> &pats) {
    Top2 t;
    if (n < k) return t;
    std::vector<unsigned> md(pats.size(), 0xFF), me(pats.size(), 0);
    for (size_t q = 0; q < pats.size(); ++q) {
        std::vector<unsigned> prev(n + 1, 0), cur(n + 1);
        for (size_t i = 1; i <= k; ++i) {
            cur[0] = (unsigned)i;
            for (size_t j = 1; j <= n; ++j) {
                unsigned v = prev[j - 1] + !((pats[q].allow[code_of(s[start + j - 1])] >> (i - 1)) & 1u);
                if (prev[j] + 1 < v) v = prev[j] + 1;
                if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
                cur[j] = v;
            }
            prev.swap(cur);
        }
        for (size_t j = 1; j <= n; ++j)
            if (prev[j] < md[q]) md[q] = prev[j], me[q] = (unsigned)j;
    }
    for (int j = 0; j < 2; ++j)
        for (size_t q = 0; q < pats.size(); ++q)
            if ((j == 0 || q != t.q[0]) && md[q] < t.d[j]) t.d[j] = (uint8_t)md[q], t.q[j] = (uint32_t)q, t.e[j] = me[q];
    return t;
}

static bool same(const Context::ReadsBest &b, size_t r, const Top2 &t, int j) { return b.query[r] == t.q[j] && b.pos[r] == t.e[j] && b.dist[r] == t.d[j]; }

static std::string random_bases(size_t n, uint64_t state) {
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    return s;
}

int main() {
    Context ctx(0);
    const size_t k = 8;
    const char *exact[] = {"ACGTTGCA", "GGATCCAT", "ACGTTGCA", "TTTTGGGG"}; // 2 equals 0
    std::vector<uint64_t> queries;
    std::vector<bitnuc_pattern> singles, pats;
    for (const char *x : exact) {
        uint64_t w = 0;
        for (size_t i = 0; i < k; ++i) w |= (uint64_t)code_of(x[i]) << (2 * i);
        queries.push_back(w);
        singles.push_back(Context::pattern_from_iupac(x).unwrap());
    }
    for (const char *x : {"ACGTNNRY", "NNTTGGCA", "ACGTNNRY", "GGSWACNT"}) pats.push_back(Context::pattern_from_iupac(x).unwrap());

    // ---- ragged
    const std::vector<size_t> lens = {140, 9, 0, 70, 7, 21, 11, 64};
    const size_t count = lens.size();
    std::vector<uint64_t> offsets = {0}, word_offsets = {0};
    for (size_t len : lens) offsets.push_back(offsets.back() + len), word_offsets.push_back(word_offsets.back() + (len + 31) / 32);
    std::string s = random_bases(offsets.back(), 0x9E3779B97F4A7C15ull);
    s.replace(offsets[0] + 60, 7, "ACGTGCA");       // read 0: query 0 (and 2) with one base deleted, across base 64
    s.replace(offsets[3] + 2, 9, "GGATCTCAT");      // read 3: query 1 with one base inserted, near its start
    s.replace(offsets[1], 9, "gACGTTGCA");          // read 1 (9 bases): query 0 in its last eight
    std::vector<uint64_t> words(word_offsets.back(), 0);
    for (size_t r = 0; r < count; ++r) {
        for (size_t i = 0; i < lens[r]; ++i) words[word_offsets[r] + i / 32] |= (uint64_t)code_of(s[offsets[r] + i]) << (2 * (i % 32));
        if (lens[r] % 32) words[word_offsets[r] + lens[r] / 32] |= ~0ull << (2 * (lens[r] % 32)); // junk in the pad bits
    }
    const auto a = ctx.reads_edist_best_batch(s, offsets, k, queries).unwrap();
    const auto p = ctx.reads_edist_best_batch_packed(words, word_offsets, offsets, k, queries).unwrap();
    const auto pa = ctx.reads_pattern_edist_best_batch(s, offsets, k, pats).unwrap();
    const auto pp = ctx.reads_pattern_edist_best_batch_packed(words, word_offsets, offsets, k, pats).unwrap();
    const auto sp = ctx.reads_pattern_edist_best_batch_packed(words, word_offsets, offsets, k, singles).unwrap();
    CHECK(a.best.query.size() == count && p.second.dist.size() == count && pp.best.pos.size() == count);
    for (size_t r = 0; r < count; ++r) {
        const Top2 t = brute(s, offsets[r], lens[r], k, singles), pt = brute(s, offsets[r], lens[r], k, pats);
        CHECK(same(a.best, r, t, 0) && same(a.second, r, t, 1) && same(p.best, r, t, 0) && same(p.second, r, t, 1));
        CHECK(same(sp.best, r, t, 0) && same(sp.second, r, t, 1));
        CHECK(same(pa.best, r, pt, 0) && same(pa.second, r, pt, 1) && same(pp.best, r, pt, 0) && same(pp.second, r, pt, 1));
    }
    CHECK(a.best.dist[0] <= 1 && a.best.pos[0] <= 67 && a.second.dist[0] <= 1); // the deletion (the equal query is the runner-up, at the latest)
    CHECK(a.best.dist[3] <= 1 && a.best.pos[3] <= 11);                           // the insertion
    CHECK(a.best.query[1] == 0 && a.best.pos[1] == 9 && a.best.dist[1] == 0);   // a read of k + 1 bases
    CHECK(a.best.dist[2] == 0xFF && a.best.dist[4] == 0xFF && a.second.query[4] == 0xFFFFFFFFu && p.best.dist[4] == 0xFF); // shorter than k: the fill

    // ---- fixed: five reads of 70 bases
    const size_t n = 70, fcount = 5;
    std::string f = random_bases(n * fcount, 0xD1B54A32D192ED03ull);
    f.replace(2 * n + 60, 7, "ACGTGCA");
    f.replace(4 * n + n - 8, 8, "GGATCCAT"); // the last read: query 1 in its last eight bases
    std::vector<uint64_t> fwords(fcount * 3, 0);
    for (size_t r = 0; r < fcount; ++r) {
        for (size_t i = 0; i < n; ++i) fwords[3 * r + i / 32] |= (uint64_t)code_of(f[r * n + i]) << (2 * (i % 32));
        fwords[3 * r + 2] |= ~0ull << (2 * (n % 32));
    }
    const auto fa = ctx.reads_edist_best(f, n, k, queries).unwrap();
    const auto fp = ctx.reads_edist_best_packed(fwords, n, fcount, k, queries).unwrap();
    const auto fpa = ctx.reads_pattern_edist_best(f, n, k, pats).unwrap();
    const auto fpp = ctx.reads_pattern_edist_best_packed(fwords, n, fcount, k, pats).unwrap();
    CHECK(fa.best.query.size() == fcount && fpp.second.dist.size() == fcount);
    for (size_t r = 0; r < fcount; ++r) {
        const Top2 t = brute(f, r * n, n, k, singles), pt = brute(f, r * n, n, k, pats);
        CHECK(same(fa.best, r, t, 0) && same(fa.second, r, t, 1) && same(fp.best, r, t, 0) && same(fp.second, r, t, 1));
        CHECK(same(fpa.best, r, pt, 0) && same(fpa.second, r, pt, 1) && same(fpp.best, r, pt, 0) && same(fpp.second, r, pt, 1));
    }
    CHECK(fa.best.dist[2] <= 1 && fa.best.pos[2] <= 67);
    CHECK(fa.best.query[4] == 1 && fa.best.pos[4] == 70 && fa.best.dist[4] == 0);

    // ---- the error mapping: an N inside a read, in a read shorter than k, too long a k, too long a read, a table of another size
    std::string bad = s;
    bad[offsets[3] + 69] = 'N';
    const auto e1 = ctx.reads_edist_best_batch(bad, offsets, k, queries);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    bad[offsets[3] + 69] = s[offsets[3] + 69];
    bad[offsets[4] + 2] = 'N';  // in a read shorter than k: ignored
    CHECK(ctx.reads_edist_best_batch(bad, offsets, k, queries).is_ok());
    CHECK(ctx.reads_edist_best_batch(s, offsets, 33, queries).is_err());
    CHECK(ctx.reads_edist_best(f, n, 33, queries).is_err());
    CHECK(ctx.reads_edist_best_packed(fwords, (size_t)BITNUC_EDIST_MAX_READ + 1, 1, k, queries).is_err());
    CHECK(ctx.reads_edist_best_batch_packed(words, std::vector<uint64_t>(word_offsets.begin(), word_offsets.end() - 1), offsets, k, queries).is_err());

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
