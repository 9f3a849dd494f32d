// The four indel-tolerant anchored methods of include/bitnuc.hpp for RAGGED batches (reads_edist_anchored_batch, reads_pattern_edist_anchored_batch and
// their _packed forms) on a small batch, against the plain dynamic programme on each read's own span, written from the definition: the admissible
// offsets of a read (START: pos_lo <= i <= min(pos_hi, last); END: pos_lo <= last - i <= pos_hi, i >= 0), the span from the first of them to k - 1
// bases behind the last, D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [no match], D[i-1][j] + 1, D[i][j-1] + 1), the smallest D[k][j] and its
// first j, the end counted from the read's start.  Small batches run on the library's host path; the C++ layer is what is under test: the argument
// order, the sizes of the vectors it allocates, the defaults, the error mapping.
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

// read [start, start + len) of s against every pattern, over its own span
static Top2 brute(const std::string &s, size_t start, size_t len, size_t k, int anchor, size_t lo, size_t hi, const std::vector<bitnuc_pattern> &pats) {
    Top2 t;
    if (len < k) return t;
    const long long last = (long long)(len - k);
    long long a, b;
    if (anchor == BITNUC_ANCHOR_END) a = last - (long long)hi < 0 ? 0 : last - (long long)hi, b = last - (long long)lo;
    else a = (long long)lo, b = (long long)hi < last ? (long long)hi : last;
    if (a > b) return t;
    const size_t first = (size_t)a, n = (size_t)(b - a) + k;
    std::vector<unsigned> md(pats.size(), 0xFF), me(pats.size(), 0);
    for (size_t q = 0; q < pats.size(); ++q) {
        std::vector<unsigned> prev(n + 1, 0), cur(n + 1);
        for (size_t i = 1; i <= k; ++i) {
            cur[0] = (unsigned)i;
            for (size_t j = 1; j <= n; ++j) {
                unsigned v = prev[j - 1] + !((pats[q].allow[code_of(s[start + first + j - 1])] >> (i - 1)) & 1u);
                if (prev[j] + 1 < v) v = prev[j] + 1;
                if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
                cur[j] = v;
            }
            prev.swap(cur);
        }
        for (size_t j = 1; j <= n; ++j)
            if (prev[j] < md[q]) md[q] = prev[j], me[q] = (unsigned)(first + j);
    }
    for (int j = 0; j < 2; ++j)
        for (size_t q = 0; q < pats.size(); ++q)
            if ((j == 0 || q != t.q[0]) && md[q] < t.d[j]) t.d[j] = (uint8_t)md[q], t.q[j] = (uint32_t)q, t.e[j] = me[q];
    return t;
}

static bool same(const Context::ReadsBest &b, size_t r, const Top2 &t, int j) { return b.query[r] == t.q[j] && b.pos[r] == t.e[j] && b.dist[r] == t.d[j]; }

int main() {
    Context ctx(0);
    const size_t k = 8;
    const std::vector<size_t> lens = {40, 9, 0, 33, 7, 21, 11, 64};
    const size_t count = lens.size();
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
    std::vector<uint64_t> offsets = {0}, word_offsets = {0};
    for (size_t len : lens) offsets.push_back(offsets.back() + len), word_offsets.push_back(word_offsets.back() + (len + 31) / 32);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    std::string s;
    for (size_t i = 0; i < offsets.back(); ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back("ACGTacgt"[(state >> 33) & 7]);
    }
    s.replace(offsets[3] + 33 - 8, 7, "ACGTGCA");   // read 3: query 0 (and 2) with one base deleted, one base in front of its end
    s.replace(offsets[7] + 2, 9, "GGATCTCAT");      // read 7: query 1 with one base inserted, near its start
    s.replace(offsets[1], 9, "gACGTTGCA");          // read 1 (9 bases): query 0 in its last eight
    std::vector<uint64_t> words(word_offsets.back(), 0);
    for (size_t r = 0; r < count; ++r) {
        for (size_t i = 0; i < lens[r]; ++i) words[word_offsets[r] + i / 32] |= (uint64_t)code_of(s[offsets[r] + i]) << (2 * (i % 32));
        if (lens[r] % 32) words[word_offsets[r] + lens[r] / 32] |= ~0ull << (2 * (lens[r] % 32)); // junk in the pad bits
    }

    const auto tail = ctx.reads_edist_anchored_batch(s, offsets, k, queries, 0, 4, BITNUC_ANCHOR_END).unwrap();                     // the last 12 bases
    const auto head = ctx.reads_edist_anchored_batch_packed(words, word_offsets, offsets, k, queries, 1, 6).unwrap();                // START by default
    const auto ptail = ctx.reads_pattern_edist_anchored_batch(s, offsets, k, pats, 0, 4, BITNUC_ANCHOR_END).unwrap();
    const auto phead = ctx.reads_pattern_edist_anchored_batch_packed(words, word_offsets, offsets, k, pats, 1, 6).unwrap();
    const auto stail = ctx.reads_pattern_edist_anchored_batch_packed(words, word_offsets, offsets, k, singles, 0, 4, BITNUC_ANCHOR_END).unwrap();
    const auto one = ctx.reads_edist_anchored_batch(s, offsets, k, queries).unwrap();                                               // the defaults: START 0 .. 0
    CHECK(tail.best.query.size() == count && head.second.dist.size() == count && phead.best.pos.size() == count);
    for (size_t r = 0; r < count; ++r) {
        const Top2 t = brute(s, offsets[r], lens[r], k, BITNUC_ANCHOR_END, 0, 4, singles), h = brute(s, offsets[r], lens[r], k, BITNUC_ANCHOR_START, 1, 6, singles);
        CHECK(same(tail.best, r, t, 0) && same(tail.second, r, t, 1) && same(head.best, r, h, 0) && same(head.second, r, h, 1));
        CHECK(same(stail.best, r, t, 0) && same(stail.second, r, t, 1));
        const Top2 pt = brute(s, offsets[r], lens[r], k, BITNUC_ANCHOR_END, 0, 4, pats), ph = brute(s, offsets[r], lens[r], k, BITNUC_ANCHOR_START, 1, 6, pats);
        CHECK(same(ptail.best, r, pt, 0) && same(ptail.second, r, pt, 1) && same(phead.best, r, ph, 0) && same(phead.second, r, ph, 1));
        const Top2 o = brute(s, offsets[r], lens[r], k, BITNUC_ANCHOR_START, 0, 0, singles);
        CHECK(same(one.best, r, o, 0) && same(one.second, r, o, 1));
    }
    // the deletion: distance 1, the end one past the seven planted bases, counted from the read's start; the equal query is the runner-up
    CHECK(tail.best.query[3] == 0 && tail.best.pos[3] == 32 && tail.best.dist[3] == 1 && tail.second.query[3] == 2 && tail.second.pos[3] == 32 && tail.second.dist[3] == 1);
    CHECK(head.best.query[7] == 1 && head.best.pos[7] == 11 && head.best.dist[7] == 1); // the insertion
    CHECK(tail.best.query[1] == 0 && tail.best.pos[1] == 9 && tail.best.dist[1] == 0);  // a read of k + 1 bases: its shortened span
    CHECK(tail.best.dist[2] == 0xFF && tail.best.dist[4] == 0xFF && tail.second.query[4] == 0xFFFFFFFFu && head.best.dist[4] == 0xFF); // no window: the fill
    CHECK(head.best.query[1] == 0 && head.best.pos[1] == 9 && head.best.dist[1] == 0); // START 1 .. 6 on nine bases: the one window at offset 1

    // the error mapping: an N inside a span, outside one, too long a k, too wide a span, a bad anchor, a table of another size
    std::string bad = s;
    bad[offsets[3] + 30] = 'N';
    const auto e1 = ctx.reads_edist_anchored_batch(bad, offsets, k, queries, 0, 4, BITNUC_ANCHOR_END);
    CHECK(e1.is_err() && e1.unwrap_err() == NucleotideError::invalid_base('N'));
    bad[offsets[3] + 30] = s[offsets[3] + 30];
    bad[offsets[3] + 3] = 'N';  // outside the span: ignored
    bad[offsets[4] + 2] = 'N';  // in a read without a window: ignored
    CHECK(ctx.reads_edist_anchored_batch(bad, offsets, k, queries, 0, 4, BITNUC_ANCHOR_END).is_ok());
    CHECK(ctx.reads_edist_anchored_batch(s, offsets, 33, queries).is_err());
    CHECK(ctx.reads_pattern_edist_anchored_batch(s, offsets, k, pats, 0, 57).is_err()); // a span of 65 bases
    CHECK(ctx.reads_edist_anchored_batch(s, offsets, k, queries, 0, 3, 2).is_err());
    CHECK(ctx.reads_edist_anchored_batch_packed(words, std::vector<uint64_t>(word_offsets.begin(), word_offsets.end() - 1), offsets, k, queries).is_err());

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
