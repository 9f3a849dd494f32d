// The four indel-tolerant anchored methods of include/bitnuc.hpp (reads_edist_anchored, reads_pattern_edist_anchored and their _packed forms) on a small
// batch, against the plain dynamic programme written from the definition: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j]
// + 1, D[i][j-1] + 1), the smallest D[k][j] over the span and its first j.  Small batches run on the library's host path; the C++ layer is what is under
// test: the argument order, the sizes of the vectors it allocates, the defaults, the error mapping.
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

// the span s[start + lo, start + lo + n) against every pattern
static Top2 brute(const std::string &s, size_t start, size_t lo, size_t n, size_t k, const std::vector<bitnuc_pattern> &pats) {
    Top2 t;
    std::vector<unsigned> md(pats.size(), 0xFF), me(pats.size(), 0);
    for (size_t q = 0; q < pats.size(); ++q) {
        std::vector<unsigned> prev(n + 1, 0), cur(n + 1);
        for (size_t i = 1; i <= k; ++i) {
            cur[0] = (unsigned)i;
            for (size_t j = 1; j <= n; ++j) {
                unsigned v = prev[j - 1] + !((pats[q].allow[code_of(s[start + lo + j - 1])] >> (i - 1)) & 1u);
                if (prev[j] + 1 < v) v = prev[j] + 1;
                if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
                cur[j] = v;
            }
            prev.swap(cur);
        }
        for (size_t j = 1; j <= n; ++j)
            if (prev[j] < md[q]) md[q] = prev[j], me[q] = (unsigned)(lo + j);
    }
    for (int j = 0; j < 2; ++j)
        for (size_t q = 0; q < pats.size(); ++q)
            if ((j == 0 || q != t.q[0]) && md[q] < t.d[j]) t.d[j] = (uint8_t)md[q], t.q[j] = (uint32_t)q, t.e[j] = me[q];
    return t;
}

static bool same(const Context::ReadsBest &b, size_t r, const Top2 &t, int j) { return b.query[r] == t.q[j] && b.pos[r] == t.e[j] && b.dist[r] == t.d[j]; }

int main() {
    Context ctx(0);
    const size_t k = 8, read_len = 40, count = 6;
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
    uint64_t state = 0x9E3779B97F4A7C15ull;
    std::string s;
    for (size_t i = 0; i < count * read_len; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    s.replace(2 * read_len + 31, 7, "ACGTGCA");   // read 2: query 0 (and 2) with one base deleted, inside the last 12 bases
    s.replace(4 * read_len + 5, 9, "GGATCTCAT");  // read 4: query 1 with one base inserted
    const std::vector<uint64_t> words = ctx.encode_fixed(s, read_len, read_len, count).unwrap();

    const auto tail = ctx.reads_edist_anchored(s, read_len, k, queries, 28).unwrap();                   // the last 12 bases: pos_hi defaults to the end
    const auto mid = ctx.reads_edist_anchored_packed(words, read_len, count, k, queries, 3, 9).unwrap(); // the span [3, 17)
    const auto ptail = ctx.reads_pattern_edist_anchored(s, read_len, k, pats, 28).unwrap();
    const auto pmid = ctx.reads_pattern_edist_anchored_packed(words, read_len, count, k, pats, 3, 9).unwrap();
    const auto stail = ctx.reads_pattern_edist_anchored(s, read_len, k, singles, 28).unwrap();
    CHECK(tail.best.query.size() == count && mid.second.dist.size() == count && pmid.best.pos.size() == count);
    for (size_t r = 0; r < count; ++r) {
        const Top2 t = brute(s, r * read_len, 28, 12, k, singles), m = brute(s, r * read_len, 3, 14, k, singles);
        CHECK(same(tail.best, r, t, 0) && same(tail.second, r, t, 1) && same(mid.best, r, m, 0) && same(mid.second, r, m, 1));
        CHECK(same(stail.best, r, t, 0) && same(stail.second, r, t, 1));
        const Top2 pt = brute(s, r * read_len, 28, 12, k, pats), pm = brute(s, r * read_len, 3, 14, k, pats);
        CHECK(same(ptail.best, r, pt, 0) && same(ptail.second, r, pt, 1) && same(pmid.best, r, pm, 0) && same(pmid.second, r, pm, 1));
    }
    // the deletion: distance 1, the end one past the seven planted bases; the equal query is the runner-up
    CHECK(tail.best.query[2] == 0 && tail.best.pos[2] == 38 && tail.best.dist[2] == 1 && tail.second.query[2] == 2 && tail.second.pos[2] == 38 && tail.second.dist[2] == 1);
    CHECK(mid.best.query[4] == 1 && mid.best.pos[4] == 14 && mid.best.dist[4] == 1); // the insertion

    // the error mapping: an N inside the span, too long a k, too wide a span
    std::string bad = s;
    bad[read_len + 30] = 'N';
    const auto e1 = ctx.reads_edist_anchored(bad, read_len, k, queries, 28);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    bad[read_len + 30] = s[read_len + 30];
    bad[read_len + 3] = 'N'; // outside the span: ignored
    CHECK(ctx.reads_edist_anchored(bad, read_len, k, queries, 28).is_ok());
    CHECK(ctx.reads_edist_anchored(s, read_len, 33, queries).is_err());
    CHECK(ctx.reads_pattern_edist_anchored_packed(words, 150, 1, k, pats).is_err()); // the whole read of 150 bases: a span above 64

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
