// The eight 3' adapter methods of include/bitnuc.hpp (reads_edist_adapter, reads_pattern_edist_adapter, their _batch and _packed forms) on small batches,
// against the definition written out: the plain DP over all rows (D[0][j] = 0, D[i][0] = i), the full candidates (i = k, any end) and the overhang candidates
// (min_overlap <= i < k at the read's end) within floor(i num / den), the smallest (misses, d, query, end), and the cut as a Levenshtein minimum over the
// starts.  Small batches run on the library's host path; the C++ layer is what is under test: the argument order, the sizes of the vectors it allocates,
// the defaults (min_overlap 3, rate 1 / 10), the error mapping.
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

typedef std::vector<std::vector<unsigned>> Table;
// rows 0 .. rows of pattern p against s[start, start + n); anchored: D[0][j] = j
static Table dp(const std::string &s, size_t start, size_t n, size_t rows, const bitnuc_pattern &p, bool anchored) {
    Table D(rows + 1, std::vector<unsigned>(n + 1, 0));
    for (size_t j = 0; j <= n; ++j) D[0][j] = anchored ? (unsigned)j : 0u;
    for (size_t i = 1; i <= rows; ++i) {
        D[i][0] = (unsigned)i;
        for (size_t j = 1; j <= n; ++j) {
            unsigned v = D[i - 1][j - 1] + !((p.allow[code_of(s[start + j - 1])] >> (i - 1)) & 1u);
            if (D[i - 1][j] + 1 < v) v = D[i - 1][j] + 1;
            if (D[i][j - 1] + 1 < v) v = D[i][j - 1] + 1;
            D[i][j] = v;
        }
    }
    return D;
}

struct Five { uint32_t adapter = 0xFFFFFFFFu, cut = 0xFFFFFFFFu, end = 0xFFFFFFFFu; uint8_t overlap = 0xFF, dist = 0xFF; };

static Five brute(const std::string &s, size_t start, size_t n, size_t k, const std::vector<bitnuc_pattern> &pats, size_t mo, size_t num, size_t den) {
    Five f;
    if (n < k) return f;
    unsigned long long best = ~0ull; // misses, d, query, end in one number
    size_t bi = 0;
    for (size_t q = 0; q < pats.size(); ++q) {
        const Table D = dp(s, start, n, k, pats[q], false);
        for (size_t i = mo; i <= k; ++i)
            for (size_t j = (i == k ? 1 : n); j <= n; ++j) {
                const unsigned d = D[i][j];
                if (d > i * num / den) continue;
                const unsigned long long key = ((unsigned long long)(k - i + d) << 48) | ((unsigned long long)d << 40) | ((unsigned long long)q << 20) | j;
                if (key < best) best = key, bi = i;
            }
    }
    if (best == ~0ull) return f;
    const size_t e = (size_t)(best & 0xFFFFF), q = (size_t)((best >> 20) & 0xFFFFF), w = e < 2 * bi - 1 ? e : 2 * bi - 1;
    unsigned low = ~0u;
    size_t at = e;
    for (size_t c = 0; c <= w; ++c) {
        const unsigned d = dp(s, start + e - c, c, bi, pats[q], true)[bi][c];
        if (d < low) low = d, at = e - c;
    }
    f.adapter = (uint32_t)q, f.cut = (uint32_t)at, f.end = (uint32_t)e, f.overlap = (uint8_t)bi, f.dist = (uint8_t)((best >> 40) & 0xFF);
    CHECK(low == f.dist);
    return f;
}

static bool same(const Context::ReadsAdapter &a, const std::vector<Five> &want) {
    if (a.adapter.size() != want.size() || a.cut.size() != want.size() || a.end.size() != want.size() || a.overlap.size() != want.size() || a.dist.size() != want.size())
        return false;
    for (size_t r = 0; r < want.size(); ++r)
        if (a.adapter[r] != want[r].adapter || a.cut[r] != want[r].cut || a.end[r] != want[r].end || a.overlap[r] != want[r].overlap || a.dist[r] != want[r].dist) return false;
    return true;
}

int main() {
    Context ctx;
    const size_t k = 12;
    const std::string ad0 = "AGATCGGAAGAG", ad1 = "CTGTCTCTTATA";
    // fixed reads of 30 bases: a full adapter inside, an exact overhang of 7, an overhang of 9 with one substitution, nothing, the second adapter's overhang
    std::vector<std::string> reads = {
        "ACGTACGTAC" + ad0 + "TTGACCAT",
        "TTGACCATGGCATTACGGATCCA" + ad0.substr(0, 7),
        "TTGACCATGGCATTACGGATC" + std::string("AGATCGCAA"),
        "TTGACCATGGCATTACGGATCCATGCATGC",
        "GGCATTACGGATCCATGCATGC" + ad1.substr(0, 8),
    };
    std::string flat;
    for (const auto &r : reads) flat += r;
    std::vector<uint64_t> queries(2, 0);
    std::vector<bitnuc_pattern> pats(2);
    const std::string *ads[2] = {&ad0, &ad1};
    for (int q = 0; q < 2; ++q) {
        for (size_t i = 0; i < k; ++i) queries[q] |= (uint64_t)code_of((*ads[q])[i]) << (2 * i);
        bitnuc_err e;
        CHECK(bitnuc_pattern_from_2bit(queries[q], k, &pats[q], &e) == BITNUC_OK);
    }
    const size_t n = 30, count = reads.size();
    const std::vector<uint8_t> bytes(flat.begin(), flat.end());
    std::vector<uint64_t> words, woff(1, 0), off(1, 0);
    for (size_t r = 0; r < count; ++r) {
        uint64_t w = 0;
        for (size_t j = 0; j < n; ++j) w |= (uint64_t)code_of(reads[r][j]) << (2 * j);
        words.push_back(w);
        woff.push_back(words.size()), off.push_back((r + 1) * n);
    }
    const size_t rules[][3] = {{3, 1, 10}, {1, 0, 1}, {5, 1, 5}, {k, 1, 1}};
    for (const auto &rule : rules) {
        std::vector<Five> want;
        for (size_t r = 0; r < count; ++r) want.push_back(brute(flat, r * n, n, k, pats, rule[0], rule[1], rule[2]));
        auto a = ctx.reads_edist_adapter(bytes, n, k, queries, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_edist_adapter_packed(words, n, count, k, queries, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_pattern_edist_adapter(bytes, n, k, pats, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_pattern_edist_adapter_packed(words, n, count, k, pats, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_edist_adapter_batch(bytes, off, k, queries, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_edist_adapter_batch_packed(words, woff, off, k, queries, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_pattern_edist_adapter_batch(bytes, off, k, pats, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
        a = ctx.reads_pattern_edist_adapter_batch_packed(words, woff, off, k, pats, rule[0], rule[1], rule[2]);
        CHECK(a.is_ok() && same(a.unwrap(), want));
    }
    // the defaults are (3, 1 / 10); by hand: read 0 carries adapter 0 in full at [10, 22), read 1 its first 7 bases at the end, read 3 nothing
    {
        auto a = ctx.reads_edist_adapter(bytes, n, k, queries);
        CHECK(a.is_ok());
        if (a.is_ok()) {
            const auto &v = a.unwrap();
            CHECK(v.adapter[0] == 0 && v.cut[0] == 10 && v.end[0] == 22 && v.overlap[0] == 12 && v.dist[0] == 0);
            CHECK(v.adapter[1] == 0 && v.cut[1] == 23 && v.end[1] == 30 && v.overlap[1] == 7 && v.dist[1] == 0);
            CHECK(v.adapter[3] == 0xFFFFFFFFu && v.cut[3] == 0xFFFFFFFFu && v.end[3] == 0xFFFFFFFFu && v.overlap[3] == 0xFF && v.dist[3] == 0xFF);
            CHECK(v.adapter[4] == 1 && v.cut[4] == 22 && v.end[4] == 30 && v.overlap[4] == 8 && v.dist[4] == 0);
        }
    }
    // the error mapping: an argument error, an invalid byte with its index, a short table
    CHECK(!ctx.reads_edist_adapter(bytes, n, k, queries, 0, 1, 10).is_ok());
    CHECK(!ctx.reads_edist_adapter(bytes, n, k, queries, 3, 2, 1).is_ok());
    {
        std::vector<uint8_t> bad = bytes;
        bad[47] = 'N';
        const auto a = ctx.reads_edist_adapter(bad, n, k, queries);
        CHECK(a.is_err() && a.unwrap_err().index == 47);
    }
    CHECK(!ctx.reads_edist_adapter_batch_packed(words, std::vector<uint64_t>(2, 0), off, k, queries).is_ok());
    std::printf(failures ? "%d FAILURES\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
