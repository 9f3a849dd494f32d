// scan_edist_start_device.h -- WHERE the alignment that ends at a given base STARTS (bitnuc_reads_edist_start*, bitnuc_ref_edist_start* and their pattern
// twins): the second stage of the indel-tolerant family.  An item is a text, a floor a, a query index and an end e; with w = min(e - a, 2k - 1) the lane
// writes the lexicographic minimum over s in [e - w, e] of (Lev(q, t[s, e)), e - s) as (dist, start = s).  No traceback matrix: the family's column step runs
// BACKWARDS from e - 1 with the query reversed and a carry-in of 1 on the horizontal delta (edist_step_device.h: edist_col_init_reversed,
// edist_col_step_anchored), so after c bases the score is D'[k][c] = Lev(q, t[e - c, e)); the running key is one v_min of (score << 6 | c) from (k << 6 | 0),
// the empty substring.  2k - 1 <= 63 columns are enough (Lev >= |c - k|, the empty substring costs k already, a tie goes to the shorter substring): the span
// the anchored kernel holds in four registers.
// ONE ITEM PER LANE, one kernel template over three geometries (G) and ASCII / packed:
//   StartFixedGeom   reads at a stride, one (query, end) per read, the floor from (anchor, pos) and read_len
//   StartBatchGeom   reads behind offsets tables, the floor from (anchor, pos) and the read's own length
//   StartRefGeom     items along one reference: 64-bit ends and starts, the floor is 0, an optional device count d_m bounds the items
// Tables: the lane loads ITS query's 16-byte entry of edist_tables_kernel's table (unchanged) and reverses each mask within k bits.
// Window: the lane gathers its w bases in front of e with edist_span_ascii / edist_span_packed (scan_edist_device.h, as they are: the aligned dwords that
// hold a walked byte, alignbyte, residue, enc4; one to three words and a funnel shift), then shifts the 128 bits left so that base e - 1 sits at the top:
// the walk takes the top two bits of a register at every step, the same bits in every lane.  Bits that come in at the bottom are steps behind w.
// Loop: wave-uniform over the wave's largest w (edist_wave_max), Eq ANDed to 0 behind a lane's own w -- such a column matches nowhere, so no D'[i][c] falls
// and the key, whose low bits grow, keeps its first minimum; a wave of equal w takes the unmasked loop.
// A skipped item (query >= nq, e > len, e < a; lanes behind the last item) has w = 0: nothing of its text or its table is loaded, no address is formed from
// its values, it writes the fill.  No LDS, no atomics but the invalid-byte latch, no scratch memory; a grid-stride loop of whole waves under the family's
// grid bound; every index along a reference is 64-bit.
#pragma once
#include "device_prims.h"
#include "edist_step_device.h" // edist_col_init_reversed, edist_col_eq, edist_col_step_anchored, edist_wave_max
#include "scan_edist_device.h" // edist_span_ascii, edist_span_packed, kEdistBlock, kEdistBlocksPerCu
#include "scan_mfma_device.h"  // trip_invalid

namespace bitnuc_dev {

// stride: bytes (ASCII) or words (packed) per read; from_end: the floor is read_len - k - pos (saturating), else pos
struct StartFixedGeom {
    using End = uint32_t;
    unsigned long long stride;
    unsigned read_len, pos, from_end, k;
};
// tab: count + 1 offsets in bases; wtab: the packed reads' first words (nullptr for ASCII)
struct StartBatchGeom {
    using End = uint32_t;
    const unsigned long long *tab, *wtab;
    unsigned pos, from_end, k;
};
// n: the reference's bases; d_m: nullptr, or a device count -- only items below min(count, *d_m) are processed and written (the kernel's
// `query` is nullptr -- every item belongs to query 0 -- or the items' query indices)
struct StartRefGeom {
    using End = unsigned long long;
    unsigned long long n;
    const unsigned long long *d_m;
    unsigned k;
};

// an item's text: at (the byte, or word, it starts at), len, the floor a
struct StartText { unsigned long long at, len, a; };
__device__ __forceinline__ unsigned long long start_floor(unsigned long long len, unsigned k, unsigned from_end, unsigned pos) {
    if (!from_end) return pos;
    const long long room = (long long)len - (long long)k - (long long)pos;
    return room > 0 ? (unsigned long long)room : 0ull;
}
template <bool PACKED> __device__ __forceinline__ StartText start_text(const StartFixedGeom &g, unsigned long long r) {
    return StartText{r * g.stride, g.read_len, start_floor(g.read_len, g.k, g.from_end, g.pos)};
}
template <bool PACKED> __device__ __forceinline__ StartText start_text(const StartBatchGeom &g, unsigned long long r) {
    const unsigned long long o0 = g.tab[r], len = g.tab[r + 1] - o0;
    return StartText{PACKED ? g.wtab[r] : o0, len, start_floor(len, g.k, g.from_end, g.pos)};
}
template <bool PACKED> __device__ __forceinline__ StartText start_text(const StartRefGeom &g, unsigned long long) { return StartText{0ull, g.n, 0ull}; }

// the lane's column against its window, W steps (wave-uniform); the lane's own window has w <= W bases, MASKED: Eq is 0 at the steps behind them.  win: the
// window with base e - 1 in the top two bits of win[3].  Returns score << 6 | c of the first minimum
template <bool MASKED>
__device__ __forceinline__ uint32_t edist_start_walk(const uint32_t (&win)[4], unsigned W, unsigned w, unsigned k, uint32_t pa, uint32_t pc, uint32_t pg, uint32_t pt) {
    uint32_t pv = ~0u, mv = 0u, sc = k, key = k << 6;
    const unsigned top = k - 1u;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
        if (16u * r >= W) break; // wave-uniform
        uint32_t codes = win[3u - r];
        const unsigned cnt = W - 16u * r < 16u ? W - 16u * r : 16u;
#pragma unroll 1
        for (unsigned s = 0; s < cnt; ++s) {
            const bool hi = (int32_t)codes < 0;
            const uint32_t lo = (uint32_t)((int32_t)(codes << 1) >> 31); // the base's low code bit as a mask
            codes <<= 2;
            const unsigned c = 16u * r + s + 1u; // the substring t[e - c, e)
            uint32_t eq = edist_col_eq(pa, pc, pg, pt, lo, hi);
            if constexpr (MASKED) eq &= c <= w ? ~0u : 0u;
            edist_col_step_anchored(eq, pv, mv, sc, top, [&key, c](uint32_t d) { key = min(key, (d << 6) + c); });
        }
    }
    return key;
}

// data: the texts (ASCII bytes at any alignment, or 8-byte aligned packed words); count items; tabs: nq entries of edist_tables_kernel (nq == 0: every item
// is skipped); query: the items' query indices (StartRefGeom: or nullptr, query 0); end, start: the geometry's End type; dist: nullptr or a byte per item.
// 1 <= k <= 32.  A bounded grid; a wave walks blocks of 64 items at the grid's stride.
template <bool PACKED, class G>
__global__ void __launch_bounds__(kEdistBlock)
edist_start_kernel(const uint8_t *__restrict__ data, unsigned long long count, const G g, const u32x4 *__restrict__ tabs, unsigned nq,
                   const uint32_t *__restrict__ query, const typename G::End *__restrict__ end, typename G::End *__restrict__ start, uint8_t *__restrict__ dist,
                   unsigned long long *__restrict__ slot) {
    using End = typename G::End;
    if constexpr (std::is_same<G, StartRefGeom>::value) {
        if (g.d_m) {
            const unsigned long long dm = *g.d_m;
            if (dm < count) count = dm;
        }
    }
    const unsigned long long step = (unsigned long long)gridDim.x * kEdistBlock;
    const unsigned lane = threadIdx.x & 63u;
    for (unsigned long long i0 = (unsigned long long)blockIdx.x * kEdistBlock + (threadIdx.x & ~63u); i0 < count; i0 += step) { // wave-uniform
        const unsigned long long i = i0 + lane;
        const bool there = i < count;
        unsigned q = 0u;
        unsigned long long e = 0ull;
        bool live = false;
        unsigned w = 0u;
        uint32_t win[4] = {0u, 0u, 0u, 0u};
        uint32_t pa = 0u, pc = 0u, pg = 0u, pt = 0u;
        if (there) {
            q = query ? query[i] : 0u;
            e = end[i];
            if (q < nq) {
                const StartText t = start_text<PACKED>(g, i);
                live = e <= t.len && e >= t.a;
                if (live) {
                    const unsigned long long room = e - t.a;
                    w = room < 2ull * g.k - 1ull ? (unsigned)room : 2u * g.k - 1u;
                    uint32_t pv, mv, sc;
                    edist_col_init_reversed(tabs[q], g.k, pa, pc, pg, pt, pv, mv, sc);
                    if (w) {
                        const unsigned long long from = e - w; // the window's first base, counted from the text's start
                        if constexpr (PACKED) {
                            edist_span_packed(reinterpret_cast<const uint64_t *>(data) + t.at + (from >> 5), (unsigned)(from & 31ull), w, win);
                        } else {
                            const unsigned long long at = t.at + from;
                            if (__builtin_expect(trip_invalid(edist_span_ascii(data + at, w, win)), 0)) rescan_bytes(data, at, w, slot);
                        }
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
                }
            }
        }
        uint32_t key;
        if (__builtin_amdgcn_ballot_w64(w != (unsigned)__builtin_amdgcn_readfirstlane((int)w)) == 0ull) { // a wave of equal w: the unmasked loop
            key = edist_start_walk<false>(win, (unsigned)__builtin_amdgcn_readfirstlane((int)w), w, g.k, pa, pc, pg, pt);
        } else {
            key = edist_start_walk<true>(win, edist_wave_max<6>(w), w, g.k, pa, pc, pg, pt);
        }
        if (there) {
            start[i] = live ? (End)(e - (key & 63u)) : (End)~(End)0;
            if (dist) dist[i] = live ? (uint8_t)(key >> 6) : (uint8_t)0xFF;
        }
    }
}

} // namespace bitnuc_dev
