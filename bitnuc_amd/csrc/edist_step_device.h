// edist_step_device.h -- the bit-parallel edit-distance column step (Myers 1999 in Hyyro's form), written ONCE for the four indel-tolerant kernels:
// scan_edist_device.h (anchored per read), scan_edist_best_device.h (the whole read), scan_edist_ref_device.h (best match and count along a reference) and
// scan_edist_hits_device.h (the hit list).  A column of one (text, query) pair is two 32-bit registers of vertical deltas (Pv, Mv) and a score D[k][j];
// per text base t_j:
//                        Eq = Peq[t_j]                      (bit i set <=> query position i matches t_j)
//                        Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
//                        Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
//                        score += bit k-1 of Ph, -= bit k-1 of Mh          (D[k][j]; starts at k = D[k][0])
//                        Ph <<= 1;  Mh <<= 1                  (no carry-in: D[0][j] = 0, the substring starts anywhere)
//                        Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
// Bits at and above k of every word are junk that never travels down (the add carries upwards, the shifts go left), so only Peq is masked to k bits and
// only bit k - 1 is tested: k = 32 needs no 1u << 32 anywhere.  Eq is two levels of selects on the base's two code bits (two three-input bit ops and a
// v_cndmask), not a lookup: the low bit toggles A -> C and G -> T by an xor, the high bit selects between the two pairs.  What a kernel does with the
// score at each base (a running key, a count, a store) is its own; with the anchored kernel's key that is 20 vector instructions per (query, base)
// (DESIGN.md 3.4 has the counts by opcode and what was tried).
// Here (the anchored forms of the start and the step, for the backward walk of scan_edist_start_device.h, stand beside them as functions of their own):
// a column's start from a table entry, Eq and the step on the column's registers (edist_col_*), the column state of U interleaved queries
// (EdistCols) with the same three on column u of it, the query groups and the wave maximum.  Every kernel that uses them compiles to the instructions
// it had when it spelled them itself, and that is kept by these rules ("The edit-distance step, written once", has what each costs):
//   - a kernel's own per-query values are members of a struct DERIVED from EdistCols, in the order its loops use them; the anchored kernel keeps arrays
//     of its own and calls the edist_col_* forms, because any struct moves it;
//   - in that kernel the lambda handed to the step captures the one key it updates by reference and the base's index by value: [&] moves it;
//   - no helper between a kernel and edist_cols_init takes the table pointer as __restrict__;
//   - the loops over four registers of sixteen codes, the trip loop along a reference and the chunk geometry are NOT here: as functions that take the
//     per-step body they compile to other code, so each kernel spells its loops around Eq and the step.
#pragma once
#include <type_traits>

#include "device_prims.h"

namespace bitnuc_dev {

constexpr int kEdistInterleave = 4;  // queries a lane runs side by side through one walk over its text
constexpr unsigned kEdistEntry = 16; // bytes of a query's table entry: Peq[A, C, G, T] masked to k bits (edist_tables_kernel, or edist_peq on the host)

// the columns of U queries side by side: the match masks and the state that travels from base to base
template <int U> struct EdistCols {
    uint32_t pa[U], pc[U], pg[U], pt[U]; // Peq[A], what the low code bit toggles (A -> C), Peq[G], (G -> T)
    uint32_t pv[U], mv[U], sc[U];
};

// ---- one column, on its registers (for a kernel that keeps them in arrays of its own)
// fresh in front of the text, from its query's table entry (wave-uniform)
__device__ __forceinline__ void edist_col_init(const u32x4 &t, unsigned k, uint32_t &pa, uint32_t &pc, uint32_t &pg, uint32_t &pt, uint32_t &pv, uint32_t &mv,
                                               uint32_t &sc) {
    pa = t.x, pc = t.x ^ t.y, pg = t.z, pt = t.z ^ t.w;
    // the masks are wave-uniform and would sit in SGPRs, of which a VALU instruction reads one: in VGPRs a select of two of them is one three-input bit op
    asm volatile("" : "+v"(pa), "+v"(pc), "+v"(pg), "+v"(pt));
    pv = ~0u, mv = 0u, sc = k;
}
// Eq at a base whose low code bit is the mask lo and whose high code bit is hi
__device__ __forceinline__ uint32_t edist_col_eq(uint32_t pa, uint32_t pc, uint32_t pg, uint32_t pt, uint32_t lo, bool hi) {
    const uint32_t eac = pa ^ (pc & lo), egt = pg ^ (pt & lo);
    return hi ? egt : eac;
}
// one base on: sc becomes D[k][j] of that base, and on_score(D[k][j]) runs between the score and the shifts.  top = k - 1
template <class OnScore> __device__ __forceinline__ void edist_col_step(uint32_t eq, uint32_t &pv, uint32_t &mv, uint32_t &sc, unsigned top, OnScore on_score) {
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv);
    uint32_t mh = pv & xh;
    sc += (ph >> top) & 1u;
    sc -= (mh >> top) & 1u;
    on_score(sc);
    ph <<= 1; // no carry-in: D[0][j] = 0
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

// ---- the same column ANCHORED at the text's first base (scan_edist_start_device.h: the backward walk from an alignment's end to its start): row 0 is
// D[0][j] = j, a carry-in of 1 on the horizontal delta -- one v_or more than edist_col_step in the shipped code (ph << 1 is also an operand of the next
// three-input bit op, so the shift and the or do not fuse).  The masks come from a table entry the LANE picked (its own query), reversed within k bits:
// they are in VGPRs without being forced there.
__device__ __forceinline__ void edist_col_init_reversed(const u32x4 &t, unsigned k, uint32_t &pa, uint32_t &pc, uint32_t &pg, uint32_t &pt, uint32_t &pv,
                                                        uint32_t &mv, uint32_t &sc) {
    const unsigned down = 32u - k;
    pa = __builtin_bitreverse32(t.x) >> down, pc = __builtin_bitreverse32(t.x ^ t.y) >> down;
    pg = __builtin_bitreverse32(t.z) >> down, pt = __builtin_bitreverse32(t.z ^ t.w) >> down;
    pv = ~0u, mv = 0u, sc = k;
}
template <class OnScore>
__device__ __forceinline__ void edist_col_step_anchored(uint32_t eq, uint32_t &pv, uint32_t &mv, uint32_t &sc, unsigned top, OnScore on_score) {
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv);
    uint32_t mh = pv & xh;
    sc += (ph >> top) & 1u;
    sc -= (mh >> top) & 1u;
    on_score(sc);
    ph = (ph << 1) | 1u; // the carry-in: D[0][j] = j
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

// ---- column u of EdistCols
template <int U> __device__ __forceinline__ void edist_cols_init(EdistCols<U> &c, int u, const u32x4 &t, unsigned k) {
    edist_col_init(t, k, c.pa[u], c.pc[u], c.pg[u], c.pt[u], c.pv[u], c.mv[u], c.sc[u]);
}
template <int U> __device__ __forceinline__ uint32_t edist_eq(const EdistCols<U> &c, int u, uint32_t lo, bool hi) {
    return edist_col_eq(c.pa[u], c.pc[u], c.pg[u], c.pt[u], lo, hi);
}
// (the forms that only count read c.sc[u] behind the step: the overload without on_score)
template <int U, class OnScore> __device__ __forceinline__ void edist_step(EdistCols<U> &c, int u, uint32_t eq, unsigned top, OnScore on_score) {
    edist_col_step(eq, c.pv[u], c.mv[u], c.sc[u], top, on_score);
}
template <int U> __device__ __forceinline__ void edist_step(EdistCols<U> &c, int u, uint32_t eq, unsigned top) {
    edist_step(c, u, eq, top, [](uint32_t) {});
}

// the queries 0 .. nq - 1 in groups: f(std::integral_constant<int, U>, q0) for the queries q0 .. q0 + U - 1, U = kEdistInterleave, then 2 and 1 for the
// remainder; wave-uniform
template <class F> __device__ __forceinline__ void edist_query_groups(unsigned nq, F f) {
    unsigned q = 0;
#pragma unroll 1
    for (; q + kEdistInterleave <= nq; q += kEdistInterleave) f(std::integral_constant<int, kEdistInterleave>{}, q);
    if (nq - q >= 2u) { f(std::integral_constant<int, 2>{}, q); q += 2u; }
    if (nq - q >= 1u) f(std::integral_constant<int, 1>{}, q);
}

// the largest x < 2^BITS among the wave's active lanes, as a wave-uniform value: a binary search with BITS ballots (no cross-lane data path)
template <unsigned BITS> __device__ __forceinline__ unsigned edist_wave_max(unsigned x) {
    unsigned m = 0;
#pragma unroll
    for (unsigned b = 1u << (BITS - 1u); b; b >>= 1)
        if (__builtin_amdgcn_ballot_w64(x >= (m | b))) m |= b;
    return m;
}

} // namespace bitnuc_dev
