// The ten per-read pattern methods of include/bitnuc.hpp (reads_pattern_best, _best2, _anchored, _best_batch, _anchored_batch and their _packed
// forms) on a small batch, against a brute force written from the definition: pdist = #{ i < k : base i not in S_i }, the best the smallest
// (distance, pattern, offset), the runner-up the same over the other patterns.  Small batches run on the library's host path; the C++ layer is what is
// under test: the argument order, the sizes of the vectors it allocates, the defaults, the error mapping.
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

static unsigned pdist(const std::string &s, size_t at, size_t k, const bitnuc_pattern &p) {
    unsigned d = 0;
    for (size_t i = 0; i < k; ++i) d += !((p.allow[code_of(s[at + i])] >> i) & 1u);
    return d;
}

struct Top2 {
    uint32_t q[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, p[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    uint8_t d[2] = {0xFF, 0xFF};
};

// the read s[start, start + len), offsets first .. first + n - 1
static Top2 brute(const std::string &s, size_t start, size_t first, size_t n, size_t k, const std::vector<bitnuc_pattern> &pats) {
    Top2 t;
    std::vector<unsigned> md(pats.size(), 0xFF), mi(pats.size(), 0);
    if (!n) return t;
    for (size_t q = 0; q < pats.size(); ++q)
        for (size_t i = first; i < first + n; ++i) {
            const unsigned d = pdist(s, start + i, k, pats[q]);
            if (d < md[q]) md[q] = d, mi[q] = (unsigned)i;
        }
    for (int j = 0; j < 2; ++j)
        for (size_t q = 0; q < pats.size(); ++q)
            if ((j == 0 || q != t.q[0]) && md[q] < t.d[j]) t.d[j] = (uint8_t)md[q], t.q[j] = (uint32_t)q, t.p[j] = mi[q];
    return t;
}

static bool same(const Context::ReadsBest &b, size_t r, const Top2 &t, int j) { return b.query[r] == t.q[j] && b.pos[r] == t.p[j] && b.dist[r] == t.d[j]; }

int main() {
    Context ctx(0);
    const size_t k = 8, read_len = 40, count = 6;
    std::vector<bitnuc_pattern> pats;
    for (const char *x : {"ACGTNNRY", "NNTTGGCA", "ACGTNNRY", "GGSWACNT"}) pats.push_back(Context::pattern_from_iupac(x).unwrap()); // 2 equals 0
    uint64_t state = 0x9E3779B97F4A7C15ull;
    std::string s;
    for (size_t i = 0; i < count * read_len; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    s.replace(2 * read_len + 5, k, "ACGTTTAC"); // an instance of patterns 0 and 2 in read 2
    s.replace(4 * read_len + 32, k, "CATTGGCA"); // an instance of pattern 1 at the last window of read 4
    const std::vector<uint64_t> words = ctx.encode_fixed(s, read_len, read_len, count).unwrap();

    // fixed-length batch
    const auto b1 = ctx.reads_pattern_best(s, read_len, k, pats).unwrap();
    const auto b1p = ctx.reads_pattern_best_packed(words, read_len, count, k, pats).unwrap();
    const auto b2 = ctx.reads_pattern_best2(s, read_len, k, pats).unwrap();
    const auto b2p = ctx.reads_pattern_best2_packed(words, read_len, count, k, pats).unwrap();
    const auto an = ctx.reads_pattern_anchored(s, read_len, k, pats, 30).unwrap();            // the last three offsets: pos_hi defaults to the end
    const auto anp = ctx.reads_pattern_anchored_packed(words, read_len, count, k, pats, 3, 6).unwrap();
    CHECK(b1.query.size() == count && b2.second.dist.size() == count && anp.best.pos.size() == count);
    for (size_t r = 0; r < count; ++r) {
        const Top2 whole = brute(s, r * read_len, 0, read_len - k + 1, k, pats);
        CHECK(same(b1, r, whole, 0) && same(b1p, r, whole, 0));
        CHECK(same(b2.best, r, whole, 0) && same(b2.second, r, whole, 1) && same(b2p.best, r, whole, 0) && same(b2p.second, r, whole, 1));
        const Top2 tail = brute(s, r * read_len, 30, 3, k, pats), mid = brute(s, r * read_len, 3, 4, k, pats);
        CHECK(same(an.best, r, tail, 0) && same(an.second, r, tail, 1) && same(anp.best, r, mid, 0) && same(anp.second, r, mid, 1));
    }
    CHECK(b2.best.query[2] == 0 && b2.best.pos[2] == 5 && b2.best.dist[2] == 0 && b2.second.query[2] == 2 && b2.second.pos[2] == 5);  // the equal pattern is the runner-up
    CHECK(an.best.query[4] == 1 && an.best.pos[4] == 32 && an.best.dist[4] == 0);

    // ragged batch: the same bases cut into reads of other lengths, one empty and one shorter than k
    const std::vector<uint64_t> lens = {40, 0, 7, 85, 8, 100};
    std::vector<uint64_t> off = {0};
    for (uint64_t n : lens) off.push_back(off.back() + n);
    CHECK(off.back() == s.size());
    std::vector<uint64_t> woff;
    const std::vector<uint64_t> bwords = ctx.encode_batch(s, off, woff).unwrap();
    const auto bb = ctx.reads_pattern_best_batch(s, off, k, pats).unwrap();
    const auto bbp = ctx.reads_pattern_best_batch_packed(bwords, woff, off, k, pats).unwrap();
    const auto ab = ctx.reads_pattern_anchored_batch(s, off, k, pats, 0, 3, BITNUC_ANCHOR_END).unwrap();
    const auto abp = ctx.reads_pattern_anchored_batch_packed(bwords, woff, off, k, pats, 1, 2).unwrap(); // the anchor defaults to START
    for (size_t r = 0; r < lens.size(); ++r) {
        const size_t len = (size_t)lens[r], nwin = len >= k ? len - k + 1 : 0;
        const Top2 whole = brute(s, (size_t)off[r], 0, nwin, k, pats);
        CHECK(same(bb, r, whole, 0) && same(bbp, r, whole, 0));
        const size_t n_end = nwin < 4 ? nwin : 4;
        const Top2 end = brute(s, (size_t)off[r], nwin - n_end, n_end, k, pats);
        CHECK(same(ab.best, r, end, 0) && same(ab.second, r, end, 1));
        const size_t n_start = nwin > 1 ? (nwin - 1 < 2 ? nwin - 1 : 2) : 0;
        const Top2 start = brute(s, (size_t)off[r], 1, n_start, k, pats);
        CHECK(same(abp.best, r, start, 0) && same(abp.second, r, start, 1));
    }
    CHECK(bb.dist[1] == 0xFF && bb.dist[2] == 0xFF && ab.second.query[1] == 0xFFFFFFFFu);

    // the error mapping: an N in a read, too long a k, tables of different sizes
    std::string bad = s;
    bad[57] = 'N';
    const auto e1 = ctx.reads_pattern_best2(bad, read_len, k, pats);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    CHECK(ctx.reads_pattern_best(s, read_len, 33, pats).is_err());
    CHECK(ctx.reads_pattern_best_batch_packed(bwords, std::vector<uint64_t>{0, 1}, off, k, pats).is_err());

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
