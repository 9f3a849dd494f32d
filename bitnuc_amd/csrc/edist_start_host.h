// edist_start_host.h -- the host side of the indel-tolerant family's SECOND STAGE: where the alignment that ends at a given base STARTS
// (bitnuc_reads_edist_start*, bitnuc_ref_edist_start* and their pattern twins; the definition is in include/bitnuc_hip.h).  An item is a text, a floor a,
// a query of k positions and an end e, a <= e <= len; with w = min(e - a, 2k - 1) the result is the lexicographic minimum over s in [e - w, e] of
// (Lev(q, t[s, e)), e - s): the smallest distance and, among the substrings that attain it, the shortest.
// No traceback matrix: the family's column step (reads_edist_host.h: edist_walk) runs BACKWARDS from e - 1 with the query reversed and a carry-in of 1 on
// the horizontal delta (row 0 is D'[0][c] = c: the substring is anchored at e, it does not start anywhere), so D'[k][c] = Lev(q, t[e - c, e)).  The running
// minimum of (D'[k][c] << 6 | c) from (k << 6 | 0) -- the empty substring -- is the answer: c <= 2k - 1 <= 63 fits the six bits.  Why 2k - 1 columns are
// enough: Lev >= |c - k|, so a substring of c >= 2k bases costs at least k, which the empty substring costs already, and a tie goes to the shorter one.
// Plain C++ on edist_peq, edist_ascii_code and edist_packed_code (no HIP): tests/c/edist_start_host_sanitize.cpp runs it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_edist_host.h" // EdistPeq, edist_peq, edist_ascii_code, edist_packed_code

namespace bitnuc_host {

// a query's match masks with the query reversed: bit i of the result is bit k - 1 - i of the mask
static inline uint32_t edist_rev_mask(uint32_t m, size_t k) {
    m = ((m >> 1) & 0x55555555u) | ((m & 0x55555555u) << 1);
    m = ((m >> 2) & 0x33333333u) | ((m & 0x33333333u) << 2);
    m = ((m >> 4) & 0x0F0F0F0Fu) | ((m & 0x0F0F0F0Fu) << 4);
    m = ((m >> 8) & 0x00FF00FFu) | ((m & 0x00FF00FFu) << 8);
    m = (m >> 16) | (m << 16);
    return m >> (32u - (unsigned)k); // 1 <= k <= 32
}
static inline EdistPeq edist_peq_reversed(const EdistPeq &p, size_t k) {
    return EdistPeq{{edist_rev_mask(p.m[0], k), edist_rev_mask(p.m[1], k), edist_rev_mask(p.m[2], k), edist_rev_mask(p.m[3], k)}};
}

// The backward walk: code_back(c) is the code of base e - c, 1 <= c <= w <= 63; rev: the reversed masks.  Returns D << 6 | c of the lexicographic minimum
// of (D'[k][c], c) over 0 <= c <= w: dist = key >> 6, start = e - (key & 63).
template <class CodeBack>
static inline uint32_t edist_start_walk(CodeBack code_back, size_t w, size_t k, const EdistPeq &rev) {
    uint32_t pv = ~0u, mv = 0u, score = (uint32_t)k, key = (uint32_t)k << 6;
    const unsigned top = (unsigned)k - 1u;
    for (size_t c = 1; c <= w; ++c) {
        const uint32_t eq = rev.m[code_back(c)];
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint32_t ph = mv | ~(xh | pv);
        uint32_t mh = pv & xh;
        score += (ph >> top) & 1u;
        score -= (mh >> top) & 1u;
        const uint32_t here = (score << 6) | (uint32_t)c;
        if (here < key) key = here;
        ph = (ph << 1) | 1u; // the carry-in: D'[0][c] = c
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
    }
    return key;
}

// an item's text: `at` is where it starts in the data (ASCII: a byte index; packed: a word index), len its bases, a its floor
struct EdistStartText { uint64_t at, len, a; };

// the floor of a read of len bases: from_end == 0 (BITNUC_ANCHOR_START): pos; else (BITNUC_ANCHOR_END): len - k - pos, saturating at 0
static inline uint64_t edist_start_floor(uint64_t len, size_t k, int from_end, size_t pos) {
    if (!from_end) return pos;
    return len >= k && len - k >= pos ? len - k - pos : 0;
}

// the bases an item walks, 0 for a skipped item (*live false): query >= nq, e > len or e < a
static inline size_t edist_start_window(const EdistStartText &t, uint64_t q, size_t nq, uint64_t e, size_t k, bool *live) {
    *live = k != 0 && q < nq && e <= t.len && e >= t.a;
    if (!*live) return 0;
    const uint64_t room = e - t.a, most = 2 * (uint64_t)k - 1;
    return (size_t)(room < most ? room : most);
}

// m items over ASCII (PACKED false: data is the bytes) or packed (data is the words) texts.  text(i): item i's EdistStartText; query_of(i): its query
// index; end[i]: its end.  Writes start[i] (the fill, all-ones, for a skipped item) and, where dist is not NULL, dist[i] (0xFF).  Returns -1, or (ASCII) the
// smallest index of an invalid byte among the walked bytes of all items, with the outputs untouched.  Nothing but the walked bases is read.
template <bool PACKED, class Q, class Text, class QueryOf, class EndT, class StartT>
static inline long long edist_start_items(const void *data, size_t m, size_t k, const Q *queries, size_t nq, Text text, QueryOf query_of, const EndT *end,
                                          StartT *start, uint8_t *dist) {
    if constexpr (!PACKED) {
        const uint8_t *s = static_cast<const uint8_t *>(data);
        long long first = -1;
        for (size_t i = 0; i < m; ++i) {
            bool live;
            const EdistStartText t = text(i);
            const size_t w = edist_start_window(t, query_of(i), nq, end[i], k, &live);
            if (!w) continue;
            const size_t from = (size_t)(t.at + end[i]) - w;
            if (first >= 0 && (long long)from >= first) continue;
            const long long bad = edist_first_invalid(s + from, w);
            if (bad >= 0 && (first < 0 || (long long)from + bad < first)) first = (long long)from + bad;
        }
        if (first >= 0) return first;
    }
    for (size_t i = 0; i < m; ++i) {
        bool live;
        const EdistStartText t = text(i);
        const uint64_t e = end[i];
        const size_t w = edist_start_window(t, query_of(i), nq, e, k, &live);
        if (!live) {
            start[i] = (StartT)~(StartT)0;
            if (dist) dist[i] = 0xFF;
            continue;
        }
        const EdistPeq rev = edist_peq_reversed(edist_peq(queries[query_of(i)], k), k);
        uint32_t key;
        if constexpr (PACKED) {
            const uint64_t *words = static_cast<const uint64_t *>(data) + t.at;
            key = edist_start_walk([&](size_t c) { return edist_packed_code(words, (size_t)(e - c)); }, w, k, rev);
        } else {
            const uint8_t *s = static_cast<const uint8_t *>(data) + t.at;
            key = edist_start_walk([&](size_t c) { return edist_ascii_code(s[e - c]); }, w, k, rev);
        }
        start[i] = (StartT)(e - (key & 63u));
        if (dist) dist[i] = (uint8_t)(key >> 6);
    }
    return -1;
}

// ---- the per-read forms: one (query, end) pair per read, the floor from (from_end, pos) and the read's length
// fixed-length reads: read r at r * read_len bytes, or at r * ceil(read_len / 32) words
template <bool PACKED, class Q>
static inline long long reads_edist_start_small(const void *data, size_t read_len, size_t count, size_t k, int from_end, size_t pos, const Q *queries, size_t nq,
                                                const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist) {
    const size_t stride = PACKED ? read_len / 32 + (read_len % 32 != 0) : read_len;
    const uint64_t a = edist_start_floor(read_len, k, from_end, pos);
    return edist_start_items<PACKED>(data, count, k, queries, nq, [&](size_t r) { return EdistStartText{(uint64_t)r * stride, read_len, a}; },
                                     [&](size_t r) { return (uint64_t)query[r]; }, end, start, dist);
}

// ragged reads behind validated tables (reads_batch_host.h); word_offsets is NULL for ASCII
template <bool PACKED, class Q>
static inline long long reads_edist_start_batch_small(const void *data, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int from_end,
                                                      size_t pos, const Q *queries, size_t nq, const uint32_t *query, const uint32_t *end, uint32_t *start,
                                                      uint8_t *dist) {
    return edist_start_items<PACKED>(data, count, k, queries, nq, [&](size_t r) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        return EdistStartText{PACKED ? word_offsets[r] : offsets[r], len, edist_start_floor(len, k, from_end, pos)};
    }, [&](size_t r) { return (uint64_t)query[r]; }, end, start, dist);
}

// ---- along a reference of n bases: m items, the floor is 0; query_index == NULL: every item belongs to query 0
template <bool PACKED, class Q>
static inline long long kmer_edist_start_small(const void *data, size_t n, size_t k, const Q *queries, size_t nq, const uint32_t *query_index, const uint64_t *end,
                                               size_t m, uint64_t *start, uint8_t *dist) {
    return edist_start_items<PACKED>(data, m, k, queries, nq, [&](size_t) { return EdistStartText{0, n, 0}; },
                                     [&](size_t i) { return query_index ? (uint64_t)query_index[i] : (uint64_t)0; }, end, start, dist);
}

} // namespace bitnuc_host
