// scan_edist_adapter_device.h -- the 3' ADAPTER per read (bitnuc_reads_edist_adapter*, _adapter_batch* and their pattern twins): of Q adapters, which one a
// read carries IN FULL anywhere or as a PREFIX that overhangs the read's end, with how many edits, and the base the alignment starts at (the cut).
//
// The whole-read kernel of scan_edist_best_device.h (one read per lane, pieces of 64 bases, EdistKeyCols and edist_step as they are, the running key
// (score << 26) + j, both layouts in one template, ASCII validated in the first query group's walk only) with three additions behind the walk:
//   the FULL candidate of a query is its running key, admissible iff key >> 26 <= allowed(k);
//   the OVERHANG candidates come from the walk's LAST COLUMN: after the read's last base (Pv, Mv) hold the vertical deltas of column n, so
//     D[i][n] = popcount(Pv & (2^i - 1)) - popcount(Mv & (2^i - 1)) for every prefix length i at once -- no second pass over the read.  The decode runs i
//     upwards (wave-uniform), d_i = d_{i-1} + bit_{i-1}(Pv) - bit_{i-1}(Mv), and keeps per query the smallest (misses << 6 | d) over min_overlap <= i < k with
//     d_i <= allowed(i), misses = k - i + d.  allowed() is non-decreasing in steps of 0 or 1 (num <= den), so it travels by value in the geometry as the
//     32-bit mask of its INCREMENTS and runs along with i in a scalar register: no device table, no division, no load.  (A byte array by value was tried
//     first: the loop's index into it made the compiler read the kernel-argument segment with one vector load per prefix length.)
//   both merge into the read's 64-bit key  misses << 48 | d << 42 | query << 26 | (end - 1)  (6 + 6 + 16 + 26 bits; overlap = k - misses + d);
//   the CUT: after all query groups the lane has one winner (q, i, e); it gathers the w = min(e, 2i - 1) bases in front of e (edist_span_ascii /
//     edist_span_packed) and runs scan_edist_start_device.h's backward walk with ITS OWN k' = i and its winner's table entry reversed within i bits
//     (edist_col_init_reversed drops the positions at and above i).  The loop is wave-uniform over the wave's largest w, masked where the lanes differ;
//     a lane without a winner has w = 0 and loads nothing.  The bytes were validated by the forward walk.
// RAGGED, masked loop: the steps behind a lane's own length run with Eq = 0 and CHANGE the column (they cannot lower D[k][j], but they are not the column
// after the read's last base), so the lane snapshots (Pv, Mv) of each interleaved query at the step j == len - 1: one compare per step, two selects per
// query.  A wave of equal lengths takes the unmasked loop and reads the final state.
// No LDS, no atomics but the invalid-byte latch, no scratch memory, 256-lane blocks, the family's bounded grid walked at its stride.
#pragma once
#include "scan_edist_best_device.h"
#include "scan_edist_start_device.h"

namespace bitnuc_dev {

// a layout's geometry (EdistBestGeom, or AnchorBatchGeom with the whole read as the window) with the adapter rule: 1 <= min_overlap <= k, full = allowed(k),
// and bit i - 1 of steps = allowed(i) - allowed(i - 1) for the prefix lengths i = 1 .. 32, allowed(i) = floor(i num / den), allowed(0) = 0
template <class G> struct EdistAdapterGeom : G {
    unsigned min_overlap, full;
    uint32_t steps;
};

// ... and of each query the column after the lane's last base (the masked loop's snapshot)
template <int U> struct EdistSnapCols : EdistKeyCols<U> { uint32_t spv[U], smv[U]; };

// edist_best_steps<U, true> with the snapshot: the column state at the step that ends at the lane's last base
template <int U>
__device__ __forceinline__ void edist_adapter_steps_masked(const uint32_t (&span)[4], unsigned cnt, unsigned j0, unsigned top, EdistSnapCols<U> &c, unsigned len) {
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        if (16u * w >= cnt) break; // wave-uniform
        uint32_t codes = span[w];
        const unsigned n16 = cnt - 16u * w < 16u ? cnt - 16u * w : 16u;
#pragma unroll 1
        for (unsigned s = 0; s < n16; ++s) {
            const uint32_t lo = 0u - (codes & 1u); // the base's low code bit as a mask
            const bool hi = (codes & 2u) != 0u;
            codes >>= 2;
            const unsigned j = j0 + 16u * w + s; // the step's end is j + 1
            const uint32_t live = j < len ? ~0u : 0u; // once per step, not per query
            const bool last = j + 1u == len;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t eq = edist_eq(c, u, lo, hi) & live;
                edist_step(c, u, eq, top, [&](uint32_t sc) { c.key[u] = min(c.key[u], (sc << kEdistBestEndBits) + j); });
                c.spv[u] = last ? c.pv[u] : c.spv[u];
                c.smv[u] = last ? c.mv[u] : c.smv[u];
            }
        }
    }
}

// Queries q0 .. q0 + U - 1 against the lane's whole read (edist_best_queries' walk and parameters), then every query's full candidate and its overhang
// candidates merged into the read's running key `best`.  len >= k, or 0 (a lane without a read: its key is discarded by the caller)
template <int U, bool MASKED, bool PACKED, class G>
__device__ __forceinline__ void edist_adapter_queries(const uint8_t *__restrict__ data, unsigned long long base, unsigned len, unsigned nmax, const EdistAdapterGeom<G> &g,
                                                      const u32x4 *__restrict__ tabs, unsigned q0, unsigned long long &best, unsigned long long *__restrict__ slot) {
    const unsigned k = g.k;
    EdistSnapCols<U> c;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        edist_cols_init(c, u, tabs[q0 + u], k);
        c.key[u] = ~0u;
        c.spv[u] = ~0u, c.smv[u] = 0u;
    }
    const unsigned top = k - 1u;
    const auto bases_of = [len](unsigned p) { return len > 64u * p ? (len - 64u * p < 64u ? len - 64u * p : 64u) : 0u; }; // the lane's bases in piece p
    const auto walk = [&](const uint32_t (&span)[4], unsigned cnt, unsigned j0) __attribute__((always_inline)) {
        if constexpr (MASKED) edist_adapter_steps_masked<U>(span, cnt, j0, top, c, len);
        else edist_best_steps<U, false>(span, cnt, j0, top, c, len);
    };
    if constexpr (PACKED) {
        const uint64_t *words = reinterpret_cast<const uint64_t *>(data) + base;
        EdistPiecePacked cur, nxt;
        edist_piece_load(words, 0u, len, cur);
#pragma unroll 1
        for (unsigned p = 0; 64u * p < nmax; ++p) {
            edist_piece_load(words, p + 1u, len, nxt); // ahead of this piece's steps (nothing behind the read)
            const uint32_t span[4] = {(uint32_t)cur.w0, (uint32_t)(cur.w0 >> 32), (uint32_t)cur.w1, (uint32_t)(cur.w1 >> 32)};
            walk(span, nmax - 64u * p < 64u ? nmax - 64u * p : 64u, 64u * p);
            cur = nxt;
        }
    } else {
        const uint8_t *a = data + base;
        const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(a) & 3u); // of every piece: they are 64 bytes apart
        EdistPieceAscii cur, nxt;
        edist_piece_load(a, bases_of(0u), cur);
#pragma unroll 1
        for (unsigned p = 0; 64u * p < nmax; ++p) {
            edist_piece_load(a + 64ull * (p + 1u), bases_of(p + 1u), nxt); // ahead of this piece's steps (nothing behind the read)
            uint32_t span[4];
            const unsigned n = bases_of(p);
            const uint32_t bad = edist_piece_codes(cur, sh, n, span);
            if (q0 == 0u && __builtin_expect(trip_invalid(bad), 0)) rescan_bytes(data, base + 64ull * p, n, slot);
            walk(span, nmax - 64u * p < 64u ? nmax - 64u * p : 64u, 64u * p);
#pragma unroll
            for (unsigned i = 0; i < 17; ++i) cur.d[i] = nxt.d[i];
        }
    }
    // the overhang decode: D[i][n] for i = 1 .. k - 1 from the last column, the smallest admissible (misses << 6 | d) per query
    uint32_t d[U], ov[U];
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = 0u, ov[u] = ~0u;
    uint32_t may = 0u; // allowed(i), wave-uniform
#pragma unroll 1
    for (unsigned i = 1; i < k; ++i) {
        may += (g.steps >> (i - 1u)) & 1u;
        const bool open = i >= g.min_overlap; // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t pv = MASKED ? c.spv[u] : c.pv[u], mv = MASKED ? c.smv[u] : c.mv[u];
            d[u] += (pv >> (i - 1u)) & 1u;
            d[u] -= (mv >> (i - 1u)) & 1u;
            if (open) {
                const uint32_t cand = ((k - i + d[u]) << 6) + d[u];
                ov[u] = d[u] <= may ? min(ov[u], cand) : ov[u];
            }
        }
    }
    constexpr uint32_t kEndMask = (1u << kEdistBestEndBits) - 1u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long q = (unsigned long long)(q0 + (unsigned)u) << kEdistBestEndBits;
        const unsigned long long fd = c.key[u] >> kEdistBestEndBits;
        const unsigned long long whole = fd <= g.full ? (fd << 48) | (fd << 42) | q | (unsigned long long)(c.key[u] & kEndMask) : ~0ull;
        const unsigned long long over =
            ov[u] != ~0u ? ((unsigned long long)(ov[u] >> 6) << 48) | ((unsigned long long)(ov[u] & 63u) << 42) | q | (unsigned long long)(len - 1u) : ~0ull;
        const unsigned long long lower = whole < over ? whole : over;
        best = best < lower ? best : lower;
    }
}

// every query against the lane's read: groups of kEdistInterleave, then of 2 and 1
template <bool MASKED, bool PACKED, class G>
__device__ __forceinline__ void edist_adapter_all_queries(const uint8_t *__restrict__ data, unsigned long long base, unsigned len, unsigned nmax,
                                                          const EdistAdapterGeom<G> &g, const u32x4 *__restrict__ tabs, unsigned long long &best,
                                                          unsigned long long *__restrict__ slot) {
    edist_query_groups(g.nq, [&](auto U, unsigned q0) { edist_adapter_queries<decltype(U)::value, MASKED, PACKED>(data, base, len, nmax, g, tabs, q0, best, slot); });
}

// The read's winner -> its five outputs.  best: the read's key, all-ones for none (the fill); base: the read's first byte or word in data.  Every active
// lane of the wave calls it: the backward walk is wave-uniform over the largest window
template <bool PACKED>
__device__ __forceinline__ void edist_adapter_finish(const uint8_t *__restrict__ data, unsigned long long base, unsigned k, const u32x4 *__restrict__ tabs,
                                                     unsigned long long best, unsigned long long r, uint32_t *__restrict__ adapter, uint32_t *__restrict__ cut,
                                                     uint32_t *__restrict__ end, uint8_t *__restrict__ overlap, uint8_t *__restrict__ dist) {
    const bool none = best == ~0ull;
    const unsigned q = (unsigned)(best >> kEdistBestEndBits) & 0xFFFFu, e = ((unsigned)best & ((1u << kEdistBestEndBits) - 1u)) + 1u;
    const unsigned d = (unsigned)(best >> 42) & 63u, i = none ? 1u : k - (unsigned)(best >> 48) + d; // the winner's prefix length
    const unsigned w = none ? 0u : (e < 2u * i - 1u ? e : 2u * i - 1u);
    uint32_t win[4] = {0u, 0u, 0u, 0u};
    uint32_t pa = 0u, pc = 0u, pg = 0u, pt = 0u;
    if (w) {
        uint32_t pv, mv, sc;
        edist_col_init_reversed(tabs[q], i, pa, pc, pg, pt, pv, mv, sc);
        const unsigned from = e - w; // the window's first base, counted from the read's start
        if constexpr (PACKED) edist_span_packed(reinterpret_cast<const uint64_t *>(data) + base + (from >> 5), from & 31u, w, win);
        else (void)edist_span_ascii(data + base + from, w, win); // validated by the forward walk
        // base e - 1 to the top: a 128-bit shift left by 2 (64 - w) bits, 2 .. 126
        unsigned long long lo = (unsigned long long)win[0] | ((unsigned long long)win[1] << 32);
        unsigned long long hi = (unsigned long long)win[2] | ((unsigned long long)win[3] << 32);
        const unsigned sh = 2u * (64u - w);
        if (sh >= 64u) {
            hi = lo << (sh - 64u);
            lo = 0ull;
        } else {
            hi = (hi << sh) | (lo >> (64u - sh));
            lo <<= sh;
        }
        win[0] = (uint32_t)lo, win[1] = (uint32_t)(lo >> 32), win[2] = (uint32_t)hi, win[3] = (uint32_t)(hi >> 32);
    }
    const unsigned W = edist_wave_max<6>(w); // wave-uniform
    uint32_t key;
    if (__builtin_amdgcn_ballot_w64(w != W) == 0ull) key = edist_start_walk<false>(win, W, w, i, pa, pc, pg, pt); // equal windows: the unmasked loop
    else key = edist_start_walk<true>(win, W, w, i, pa, pc, pg, pt);
    adapter[r] = none ? 0xFFFFFFFFu : q;
    cut[r] = none ? 0xFFFFFFFFu : e - (key & 63u);
    end[r] = none ? 0xFFFFFFFFu : e;
    overlap[r] = none ? (uint8_t)0xFF : (uint8_t)i;
    dist[r] = none ? (uint8_t)0xFF : (uint8_t)d;
}

// data: the reads (ASCII bytes at any alignment, or 8-byte aligned packed words); count >= 1, 1 <= k <= 32, 1 <= nq <= 65536; tabs: nq entries of
// edist_tables_kernel; reads of at most 2^26 bases; fixed: k <= g.len.  A bounded grid; a lane walks reads at the grid's stride.  G: the layout policy
// (EdistBestGeom: a fixed stride and length; AnchorBatchGeom: tables, the whole read as the window).
template <bool PACKED, class G>
__global__ void __launch_bounds__(kEdistBlock)
reads_edist_adapter_kernel(const uint8_t *__restrict__ data, unsigned long long count, const EdistAdapterGeom<G> g, const u32x4 *__restrict__ tabs,
                           uint32_t *__restrict__ adapter, uint32_t *__restrict__ cut, uint32_t *__restrict__ end, uint8_t *__restrict__ overlap,
                           uint8_t *__restrict__ dist, unsigned long long *__restrict__ slot) {
    const unsigned long long step = (unsigned long long)gridDim.x * kEdistBlock;
    unsigned long long r = (unsigned long long)blockIdx.x * kEdistBlock + threadIdx.x;
    if constexpr (!G::kRagged) {
        for (; r < count; r += step) {
            unsigned long long best = ~0ull;
            edist_adapter_all_queries<false, PACKED>(data, r * g.stride, g.len, g.len, g, tabs, best, slot);
            edist_adapter_finish<PACKED>(data, r * g.stride, g.k, tabs, best, r, adapter, cut, end, overlap, dist);
        }
    } else {
        AnchorEntries ahead{0, 0, 0}; // the table entries of the lane's next read
        if (r < count) ahead = anchored_entries<PACKED>(g, r);
        for (; r < count; r += step) {
            const AnchorLane L = anchored_lane<PACKED>(g, ahead);
            const unsigned len = L.n ? L.n + g.k - 1u : 0u; // the read's bases; 0 where it is shorter than k: nothing of it is loaded or validated
            if (r + step < count) ahead = anchored_entries<PACKED>(g, r + step);
            const unsigned nmax = edist_wave_max<kEdistBestEndBits + 1>(len); // wave-uniform; 0: no lane of the wave has a read of k bases
            unsigned long long best = ~0ull;
            if (__builtin_amdgcn_ballot_w64(len != nmax) == 0ull) { // a wave of equal lengths: the fixed layout's loop
                if (nmax) edist_adapter_all_queries<false, PACKED>(data, L.base, len, nmax, g, tabs, best, slot);
            } else {
                edist_adapter_all_queries<true, PACKED>(data, L.base, len, nmax, g, tabs, best, slot);
                if (!len) best = ~0ull; // the masked steps of a lane without a read made keys of no read
            }
            edist_adapter_finish<PACKED>(data, L.base, g.k, tabs, best, r, adapter, cut, end, overlap, dist);
        }
    }
}

} // namespace bitnuc_dev
