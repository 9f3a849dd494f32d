// The four kmer_*edist_hits* methods of include/bitnuc.hpp (kmer_edist_hits, its _packed form and the pattern twins) on a small reference, against the
// plain dynamic programme written from the definition: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1),
// E(j) = D[k][j]; the hits are the j with E(j) <= tau in ascending order.  A small reference runs on the library's host path; the C++ layer is what
// is under test: the argument order, the sizes of the vectors it allocates, the error mapping.
#include "bitnuc.hpp"

#include <algorithm>
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

static bool agree(const std::vector<uint64_t> &end, const std::vector<uint8_t> *dist, const std::string &s, size_t k, const bitnuc_pattern &p, unsigned tau) {
    const std::vector<unsigned> e = ends_of(s, k, p);
    size_t r = 0;
    for (size_t j = 0; j < e.size(); ++j) {
        if (e[j] > tau) continue;
        if (r >= end.size() || end[r] != j + 1 || (dist && (r >= dist->size() || (*dist)[r] != e[j]))) return false;
        ++r;
    }
    return r == end.size() && (!dist || dist->size() == r);
}

int main() {
    Context ctx(0);
    const size_t k = 8, n = 300;
    const char *exact = "ACGTTGCA";
    uint64_t query = 0;
    for (size_t i = 0; i < k; ++i) query |= (uint64_t)code_of(exact[i]) << (2 * i);
    const bitnuc_pattern single = Context::pattern_from_iupac(exact).unwrap();
    const bitnuc_pattern pat = Context::pattern_from_iupac("ACGTNNRY").unwrap();
    uint64_t state = 0x9E3779B97F4A7C15ull;
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    s.replace(100, 7, "ACGTGCA");   // the query with one base deleted
    s.replace(200, 9, "ACGTTAGCA"); // the query with one base inserted
    s.replace(260, 8, "ACGTTGCA");  // an exact copy: a run of ends at tau = 1
    const std::vector<uint64_t> words = ctx.encode_alloc(s).unwrap();

    for (unsigned tau : {0u, 1u, 2u, 8u}) {
        std::vector<uint8_t> d, dp, ds, dq;
        const auto h = ctx.kmer_edist_hits(s, k, query, tau, &d).unwrap();
        const auto hp = ctx.kmer_edist_hits_packed(words, n, k, query, tau, &dp).unwrap();
        CHECK(agree(h, &d, s, k, single, tau) && agree(hp, &dp, s, k, single, tau));
        CHECK(agree(ctx.kmer_edist_hits(s, k, query, tau).unwrap(), nullptr, s, k, single, tau)); // without hit_dist
        const auto hs = ctx.kmer_pattern_edist_hits(s, k, single, tau, &ds).unwrap();
        CHECK(hs == h && ds == d); // a singleton pattern: the exact form's result
        const auto pq = ctx.kmer_pattern_edist_hits(s, k, pat, tau, &dq).unwrap();
        const auto pqp = ctx.kmer_pattern_edist_hits_packed(words, n, k, pat, tau).unwrap();
        CHECK(agree(pq, &dq, s, k, pat, tau) && pqp == pq);
        CHECK(h.size() == ctx.kmer_edist_count_multi(s, k, {query}, {tau}).unwrap()[0]);
        CHECK(std::find(h.begin(), h.end(), (uint64_t)268) != h.end()); // the exact copy ends at base 268
        if (tau == 8) CHECK(h.size() == n);
    }

    // no windows: an empty list; the error mapping: an N, too long a k, too few words
    CHECK(ctx.kmer_edist_hits(std::string("ACG"), k, query, 8).unwrap().empty());
    std::string bad = s;
    bad[150] = 'N';
    const auto e1 = ctx.kmer_edist_hits(bad, k, query, 1);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    CHECK(ctx.kmer_pattern_edist_hits(bad, k, pat, 1).is_err());
    CHECK(ctx.kmer_edist_hits(s, 33, query, 1).is_err());
    CHECK(ctx.kmer_edist_hits_packed(words, 32 * words.size() + 1, k, query, 1).is_err());

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("kmer edist hits hpp ok\n");
    return 0;
}
