// The eight kmer_*edist_* methods of include/bitnuc.hpp (kmer_edist_best, kmer_edist_count_multi, their _packed forms and the pattern twins) on a small
// reference, against the plain dynamic programme written from the definition: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match],
// D[i-1][j] + 1, D[i][j-1] + 1), E(j) = D[k][j].  A small reference runs on the library's host path; the C++ layer is what is under test: the
// argument order, the sizes of the vectors it allocates, the error mapping.
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

// E(1) .. E(n) of one pattern
static std::vector<unsigned> ends_of(const std::string &s, size_t k, const bitnuc_pattern &p) {
    const size_t n = s.size();
    std::vector<unsigned> prev(n + 1, 0), cur(n + 1);
    for (size_t i = 1; i <= k; ++i) {
        cur[0] = (unsigned)i;
        for (size_t j = 1; j <= n; ++j) {
            unsigned v = prev[j - 1] + !((p.allow[code_of(s[j - 1])] >> (i - 1)) & 1u);
            if (prev[j] + 1 < v) v = prev[j] + 1;
            if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
            cur[j] = v;
        }
        prev.swap(cur);
    }
    return std::vector<unsigned>(prev.begin() + 1, prev.end());
}

static bool agree(const Context::EndDist &got, const std::vector<uint64_t> &counts, const std::string &s, size_t k, const std::vector<bitnuc_pattern> &pats,
                  const std::vector<uint32_t> &taus) {
    if (got.first.size() != pats.size() || got.second.size() != pats.size() || counts.size() != pats.size()) return false;
    for (size_t q = 0; q < pats.size(); ++q) {
        const std::vector<unsigned> e = ends_of(s, k, pats[q]);
        unsigned best = 0xFF;
        uint64_t at = 0, cnt = 0;
        for (size_t j = 0; j < e.size(); ++j) {
            if (e[j] < best) best = e[j], at = j + 1;
            cnt += e[j] <= taus[q];
        }
        if (got.first[q] != at || got.second[q] != best || counts[q] != cnt) return false;
    }
    return true;
}

int main() {
    Context ctx(0);
    const size_t k = 8, n = 300;
    const char *exact[] = {"ACGTTGCA", "GGATCCAT", "TTTTGGGG"};
    std::vector<uint64_t> queries;
    std::vector<bitnuc_pattern> singles, pats;
    for (const char *x : exact) {
        uint64_t w = 0;
        for (size_t i = 0; i < k; ++i) w |= (uint64_t)code_of(x[i]) << (2 * i);
        queries.push_back(w);
        singles.push_back(Context::pattern_from_iupac(x).unwrap());
    }
    for (const char *x : {"ACGTNNRY", "NNTTGGCA", "GGSWACNT"}) pats.push_back(Context::pattern_from_iupac(x).unwrap());
    const std::vector<uint32_t> taus = {1, 0, 3};
    uint64_t state = 0x9E3779B97F4A7C15ull;
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    s.replace(100, 7, "ACGTGCA");   // query 0 with one base deleted
    s.replace(200, 9, "GGATCTCAT"); // query 1 with one base inserted
    const std::vector<uint64_t> words = ctx.encode_alloc(s).unwrap();

    const auto b = ctx.kmer_edist_best(s, k, queries).unwrap();
    const auto bp = ctx.kmer_edist_best_packed(words, n, k, queries).unwrap();
    const auto c = ctx.kmer_edist_count_multi(s, k, queries, taus).unwrap();
    const auto cp = ctx.kmer_edist_count_multi_packed(words, n, k, queries, taus).unwrap();
    CHECK(agree(b, c, s, k, singles, taus) && agree(bp, cp, s, k, singles, taus));
    CHECK(b.second[0] <= 1 && b.second[1] <= 1);
    CHECK(b.second[0] == 0 || (b.first[0] <= 107 && b.second[0] == 1)); // the deletion: distance 1 at the latest one past the seven planted bases
    const auto sb = ctx.kmer_pattern_edist_best(s, k, singles).unwrap();
    const auto sc = ctx.kmer_pattern_edist_count_multi(s, k, singles, taus).unwrap();
    CHECK(sb == b && sc == c); // singleton patterns: the exact forms' results
    const auto pb = ctx.kmer_pattern_edist_best(s, k, pats).unwrap();
    const auto pbp = ctx.kmer_pattern_edist_best_packed(words, n, k, pats).unwrap();
    const auto pc = ctx.kmer_pattern_edist_count_multi(s, k, pats, taus).unwrap();
    const auto pcp = ctx.kmer_pattern_edist_count_multi_packed(words, n, k, pats, taus).unwrap();
    CHECK(agree(pb, pc, s, k, pats, taus) && agree(pbp, pcp, s, k, pats, taus));

    // no windows: the fill and zeros; the error mapping: an N, too long a k, one tau too few
    const auto none = ctx.kmer_edist_best(std::string("ACG"), k, queries).unwrap();
    CHECK(none.first[0] == UINT64_MAX && none.second[2] == 0xFF);
    CHECK(ctx.kmer_edist_count_multi(std::string("ACG"), k, queries, taus).unwrap() == std::vector<uint64_t>(3, 0));
    std::string bad = s;
    bad[150] = 'N';
    const auto e1 = ctx.kmer_edist_best(bad, k, queries);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    CHECK(ctx.kmer_pattern_edist_count_multi(bad, k, pats, taus).is_err());
    CHECK(ctx.kmer_edist_best(s, 33, queries).is_err());
    CHECK(ctx.kmer_edist_count_multi(s, k, queries, {1, 2}).is_err());
    CHECK(ctx.kmer_edist_best_packed(words, 32 * words.size() + 1, k, queries).is_err());

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("kmer edist hpp ok\n");
    return 0;
}
