// reads_edist_adapter_host.h -- the 3' ADAPTER per read below the host cutoff (bitnuc_reads_edist_adapter / _packed / _batch / _batch_packed and their
// pattern twins; the definition is in include/bitnuc_hip.h): of the queries, which one a read carries in FULL anywhere (i = k, any end j) or as a PREFIX
// of min_overlap <= i < k positions that OVERHANGS the read's end (j = n), within allowed(i) = floor(i num / den) edits; the winner is the smallest
// (misses, d, query, j) with d = D[i][j], misses = k - (i - d); then the cut: where that alignment starts.
// The family's bit-parallel walk (reads_edist_host.h's recurrence, one 32-bit column per (read, query)) with the LAST COLUMN KEPT: after the read's last
// base (Pv, Mv) are the vertical deltas of column n, so D[i][n] = D[i - 1][n] + bit_{i-1}(Pv) - bit_{i-1}(Mv) from D[0][n] = 0 gives every prefix length at
// once.  The cut is edist_start_host.h's backward walk with k' = i and the query's masks reversed within i bits, over min(e, 2i - 1) bases.
// Plain C++ for both layouts and both query kinds (no HIP): tests/c/reads_edist_adapter_host_sanitize.cpp runs it under ASan + UBSan.  The tests' oracle
// is the plain DP over all rows with a direct Levenshtein minimum for the cut, so the two are independent.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "edist_start_host.h" // edist_rev_mask, edist_start_walk; reads_edist_host.h's EdistPeq, edist_peq, the codes and edist_first_invalid through it

namespace bitnuc_host {

// allowed[i] = floor(i num / den) for the prefix lengths i = 0 .. 32 (num <= den, den >= 1: at most i, and exact in 128 bits)
struct AdapterRule { size_t min_overlap; uint8_t allowed[33]; };
static inline AdapterRule adapter_rule(size_t min_overlap, size_t num, size_t den) {
    AdapterRule r{min_overlap, {}};
    for (size_t i = 0; i <= 32; ++i) r.allowed[i] = (uint8_t)((unsigned __int128)i * num / den);
    return r;
}

constexpr uint64_t kAdapterNone = ~(uint64_t)0;

// n >= k bases of a read (code_at(j), 0-based) against every query: the smallest key  misses << 48 | d << 42 | query << 26 | (end - 1)  over the admissible
// candidates, or kAdapterNone.  1 <= k <= 32, n <= 2^26, nq <= 65536
template <class Q, class CodeAt>
static inline uint64_t adapter_read(CodeAt code_at, size_t n, size_t k, const Q *queries, size_t nq, const AdapterRule &rule) {
    uint64_t best = kAdapterNone;
    const unsigned top = (unsigned)k - 1u;
    for (size_t q = 0; q < nq; ++q) {
        const EdistPeq p = edist_peq(queries[q], k);
        uint32_t pv = ~0u, mv = 0u, score = (uint32_t)k, low = ~0u;
        size_t end = 0;
        for (size_t j = 0; j < n; ++j) {
            const uint32_t eq = p.m[code_at(j)];
            const uint32_t xv = eq | mv;
            const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
            uint32_t ph = mv | ~(xh | pv);
            uint32_t mh = pv & xh;
            score += (ph >> top) & 1u;
            score -= (mh >> top) & 1u;
            if (score < low) low = score, end = j + 1; // ends come in ascending order: the first stays
            ph <<= 1; // no carry-in: D[0][j] = 0
            mh <<= 1;
            pv = mh | ~(xv | ph);
            mv = ph & xv;
        }
        const uint64_t qbits = (uint64_t)q << 26;
        if (low <= rule.allowed[k]) { // the full candidate: misses = d
            const uint64_t c = ((uint64_t)low << 48) | ((uint64_t)low << 42) | qbits | (uint64_t)(end - 1);
            if (c < best) best = c;
        }
        uint32_t d = 0; // D[i][n], from the last column
        for (size_t i = 1; i < k; ++i) {
            d += (pv >> (i - 1)) & 1u;
            d -= (mv >> (i - 1)) & 1u;
            if (i < rule.min_overlap || d > rule.allowed[i]) continue;
            const uint64_t c = ((uint64_t)(k - i + d) << 48) | ((uint64_t)d << 42) | qbits | (uint64_t)(n - 1);
            if (c < best) best = c;
        }
    }
    return best;
}

// the winner's key -> the read's five outputs (which hold the fill already).  code_at: as above
template <class Q, class CodeAt>
static inline void adapter_store(uint64_t key, CodeAt code_at, size_t k, const Q *queries, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap,
                                 uint8_t *dist) {
    if (key == kAdapterNone) return;
    const size_t q = (size_t)(key >> 26) & 0xFFFF, e = (size_t)(key & 0x3FFFFFF) + 1, d = (size_t)(key >> 42) & 63, i = k - (size_t)(key >> 48) + d;
    const size_t w = e < 2 * i - 1 ? e : 2 * i - 1;
    const EdistPeq p = edist_peq(queries[q], k);
    const EdistPeq rev{{edist_rev_mask(p.m[0], i), edist_rev_mask(p.m[1], i), edist_rev_mask(p.m[2], i), edist_rev_mask(p.m[3], i)}}; // the PREFIX, backwards
    const uint32_t sk = edist_start_walk([&](size_t c) { return code_at(e - c); }, w, i, rev);
    *adapter = (uint32_t)q, *cut = (uint32_t)(e - (sk & 63u)), *end = (uint32_t)e, *overlap = (uint8_t)i, *dist = (uint8_t)d;
}

// no admissible candidate: UINT32_MAX x 3, 0xFF x 2
static inline void adapter_fill(size_t count, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist) {
    for (size_t r = 0; r < count; ++r) adapter[r] = cut[r] = end[r] = 0xFFFFFFFFu, overlap[r] = dist[r] = 0xFF;
}

// count reads: read(r) gives {bytes or words of read r, its bases}; a read of fewer than k bases keeps the fill and is not looked at
template <bool PACKED, class Q, class Read>
static inline void adapter_reads(size_t count, size_t k, const Q *queries, size_t nq, const AdapterRule &rule, Read read, uint32_t *adapter, uint32_t *cut,
                                 uint32_t *end, uint8_t *overlap, uint8_t *dist) {
    adapter_fill(count, adapter, cut, end, overlap, dist);
    for (size_t r = 0; r < count; ++r) {
        const auto t = read(r);
        const size_t len = t.second;
        if (len < k) continue;
        const auto code_at = [&](size_t j) {
            if constexpr (PACKED) return edist_packed_code(t.first, j);
            else return edist_ascii_code(t.first[j]);
        };
        adapter_store(adapter_read(code_at, len, k, queries, nq, rule), code_at, k, queries, adapter + r, cut + r, end + r, overlap + r, dist + r);
    }
}

template <class T> struct AdapterText { const T *first; size_t second; };

// ---- fixed-length reads (1 <= k <= min(read_len, 32), nq >= 1).  Packed: ceil(read_len / 32) words per read, bits above a read's last base are never
// looked at.  ASCII: -1 with the outputs written, or the index of the first invalid byte of the buffer (outputs untouched)
template <class Q>
static inline void reads_edist_adapter_packed_small(const uint64_t *words, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, const AdapterRule &rule,
                                                    uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist) {
    const size_t wpr = read_len / 32 + (read_len % 32 != 0);
    adapter_reads<true>(count, k, queries, nq, rule, [&](size_t r) { return AdapterText<uint64_t>{words + r * wpr, read_len}; }, adapter, cut, end, overlap, dist);
}
template <class Q>
static inline long long reads_edist_adapter_small(const uint8_t *reads, size_t read_len, size_t count, size_t k, const Q *queries, size_t nq, const AdapterRule &rule,
                                                  uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist) {
    const long long bad = edist_first_invalid(reads, count * read_len);
    if (bad >= 0) return bad;
    adapter_reads<false>(count, k, queries, nq, rule, [&](size_t r) { return AdapterText<uint8_t>{reads + r * read_len, read_len}; }, adapter, cut, end, overlap, dist);
    return -1;
}

// ---- the RAGGED batch: reads behind reads_batch_host.h's validated tables.  A read of fewer than k bases keeps the fill; none of its bytes or words is
// read or validated
template <class Q>
static inline void reads_edist_adapter_batch_packed_small(const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                          const Q *queries, size_t nq, const AdapterRule &rule, uint32_t *adapter, uint32_t *cut, uint32_t *end,
                                                          uint8_t *overlap, uint8_t *dist) {
    adapter_reads<true>(count, k, queries, nq, rule, [&](size_t r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        return AdapterText<uint64_t>{len < k ? nullptr : words + word_offsets[r], len};
    }, adapter, cut, end, overlap, dist);
}
template <class Q>
static inline long long reads_edist_adapter_batch_small(const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const Q *queries, size_t nq,
                                                        const AdapterRule &rule, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist) {
    for (size_t r = 0; r < count; ++r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        if (len < k) continue;
        const long long bad = edist_first_invalid(seq + offsets[r], len);
        if (bad >= 0) return (long long)offsets[r] + bad;
    }
    adapter_reads<false>(count, k, queries, nq, rule, [&](size_t r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        return AdapterText<uint8_t>{len < k ? nullptr : seq + offsets[r], len};
    }, adapter, cut, end, overlap, dist);
    return -1;
}

} // namespace bitnuc_host
