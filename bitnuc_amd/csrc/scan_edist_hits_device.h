// scan_edist_hits_device.h -- the INDEL-TOLERANT HIT LIST along a reference (bitnuc_kmer_edist_hits* and its bitnuc_kmer_pattern_edist_hits* twins): with
// E(j) = D[k][j] of scan_edist_ref_device.h (the edit distance of the query to the best substring of the reference that ends at base j; `end` j is one
// past the last aligned base, 1 <= j <= n),
//   *n_hits = #{ j : E(j) <= tau } (what the count returns for the same query and tau; it may exceed cap),
//   end[0 .. min(cap, *n_hits)) = those j in ascending order, hit_dist[r] = E(end[r]) (hit_dist may be NULL).
// Neighbouring ends of a good match are hits too (E(j +- 1) <= E(j) + 1), so an exact copy shows as a run of up to 2 tau + 1 ends; the list is not
// collapsed to local minima.  One query per call, a host value: its 16-byte table entry (what edist_tables_kernel would write) is built on the host
// (edist_peq) and travels as a kernel argument -- nothing is uploaded.
//
// Three stream-ordered launches, no workgroup ever waits for another (scan_hits_device.h's plan, with CHUNKS as the scan's entries):
//   1. kmer_edist_hits_kernel<PACKED, false>: the count pass.  kmer_edist_kernel's chunk walk for one query -- one chunk of kEdistRefChunk = 1024
//      reported columns per lane behind the 64-column lead-in, `lead` for the host chunk loops, fast and general steps, the next trip's loads issued
//      before the current trip's steps, a bounded grid walked at its stride -- writes the lane's number of hits (<= 1024) to counts[chunk] and to
//      raw[chunk].  No atomics.  An invalid ASCII byte is latched here only.
//   2. hits_scan_tiles_kernel + hits_scan_top_kernel, unchanged: the exclusive scan of counts[] (977 K entries at 10^9 bases), which also writes *n_hits.
//      raw[] keeps the per-chunk counts: the emit pass has to know which chunks hold a hit.
//   3. kmer_edist_hits_kernel<PACKED, true>: the emit pass (not launched for cap == 0).  A lane whose chunk counted no hit, or whose first rank is at or
//      beyond cap, does not walk it: a wave of 64 such chunks only reads its counts.  A lane with hits repeats the walk over the same bytes with the
//      same step instructions and writes end / hit_dist at offset(chunk) + its running rank as the hits appear, nothing at or beyond cap.  The
//      reported end is column - lead + 1 + pos_base.  Chunks are in column order and a lane's hits come in column order: ascending without a sort.
// THE EMIT STEP'S STORE is a predicated store inside the step (a branch around two stores and the rank's increment), not a per-trip 64-bit hit mask
// emitted after the trip: hit_dist needs the score AT the hit, which a mask does not carry (64 scores of 6 bits would be 12 more registers per lane
// or a second walk), the branch is skipped by the whole wave where no lane has a hit in that step (the sparse case: the walk then costs what the count
// pass's costs), and in the dense case the per-lane stores are uncoalesced either way (lanes are 1024 ends apart).  The step loop is not unrolled, so
// the store exists 4 times per trip form, not 64 times.
// All position arithmetic is 64-bit.  Deterministic (no atomics but the invalid byte's latch, no ticket, no LDS) and capturable.
#pragma once
#include "device_prims.h"
#include "scan_edist_ref_device.h" // the chunks and trips: kEdistRefChunk ..., edist_ref_load, edist_ref_codes; the step through edist_step_device.h
#include "scan_hits_device.h"      // kHitsTile, the scan

namespace bitnuc_dev {

// what one lane reports beside its column (EdistCols<1>).  Count: acc = the reported columns with score <= tau.  Emit: rank = where the next hit goes
struct EdistHitsState : EdistCols<1> { uint32_t tau, acc; unsigned long long rank; };

// the 64 steps of a trip whose first column has the end e0.  FAST: every column is reported; otherwise those with lo <= (index in the trip) < lo + width
template <bool EMIT, bool FAST>
__device__ __forceinline__ void edist_hits_steps(const uint32_t (&codes)[4], unsigned top, EdistHitsState &st, unsigned lo, unsigned width, unsigned long long e0,
                                                 unsigned long long *__restrict__ pos, uint8_t *__restrict__ hd, unsigned long long cap) {
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        uint32_t c = codes[w];
#pragma unroll 1
        for (unsigned s = 0; s < 16; ++s) {
            const uint32_t lowm = 0u - (c & 1u); // the base's low code bit as a mask
            const bool hi = (c & 2u) != 0u;
            c >>= 2;
            const unsigned tl = 16u * w + s;
            if constexpr (EMIT) {
                edist_step(st, 0, edist_eq(st, 0, lowm, hi), top, [&](uint32_t sc) {
                    bool hit = sc <= st.tau;
                    if constexpr (!FAST) hit = hit && (tl - lo) < width;
                    if (hit) {
                        if (st.rank < cap) {
                            pos[st.rank] = e0 + tl;
                            if (hd) hd[st.rank] = (uint8_t)sc;
                        }
                        ++st.rank;
                    }
                });
            } else {
                edist_step(st, 0, edist_eq(st, 0, lowm, hi), top);
                bool hit = st.sc[0] <= st.tau;
                if constexpr (!FAST) hit = hit && (tl - lo) < width;
                st.acc += hit ? 1u : 0u;
            }
        }
    }
}

// the lane's walk over the columns [s, r1) of which [r0, r1) are reported, r0 < r1 <= n; returns the number of hits (count pass)
template <bool PACKED, bool EMIT>
__device__ __forceinline__ uint32_t edist_hits_walk(const uint8_t *__restrict__ data, unsigned long long n, unsigned long long s, unsigned long long r0,
                                                    unsigned long long r1, unsigned k, const u32x4 &tab, unsigned tau, unsigned long long rank,
                                                    unsigned long long ebase, unsigned long long *__restrict__ pos, uint8_t *__restrict__ hd,
                                                    unsigned long long cap, unsigned long long *__restrict__ slot) {
    EdistHitsState st;
    edist_cols_init(st, 0, tab, k);
    st.tau = tau, st.acc = 0u, st.rank = rank;
    const unsigned top = k - 1u;
    const unsigned units = (unsigned)((r1 - s + kEdistRefTrip - 1) / kEdistRefTrip);
    auto raw = edist_ref_load<PACKED>(data, s, n);
    for (unsigned u = 0; u < units; ++u) {
        const unsigned long long b = s + (unsigned long long)u * kEdistRefTrip;
        uint32_t codes[4];
        edist_ref_codes<!EMIT>(raw, data, b, n, slot, codes); // ASCII bytes are validated (and latched) by the count pass only
        if (u + 1u < units) raw = edist_ref_load<PACKED>(data, b + kEdistRefTrip, n); // b + 64 < r1 <= n
        if (b >= r0 && b + kEdistRefTrip <= r1) {
            edist_hits_steps<EMIT, true>(codes, top, st, 0u, 0u, b + ebase, pos, hd, cap);
        } else {
            const unsigned lo = r0 > b ? (r0 - b < kEdistRefTrip ? (unsigned)(r0 - b) : kEdistRefTrip) : 0u;
            const unsigned hi = r1 - b < kEdistRefTrip ? (unsigned)(r1 - b) : kEdistRefTrip; // r1 > b
            edist_hits_steps<EMIT, false>(codes, top, st, lo, hi - lo, b + ebase, pos, hd, cap);
        }
    }
    return st.acc;
}

// data: n >= 1 bases (ASCII bytes at any alignment, or 8-byte aligned packed words); lead < n columns are run but not reported, lead <= kEdistRefLead
// and, packed, a multiple of 32; 1 <= k <= 32; tab: the query's entry.  counts / raw: one u32 per chunk of the n - lead reported columns; tile_off: the
// scan's tile offsets (emit).  Count pass: counts[c] = raw[c] = chunk c's hits.  Emit pass: counts[] scanned, raw[] as the count pass left it.
// blockDim.x == kEdistRefBlock; any grid: chunks are walked at the grid's stride.
template <bool PACKED, bool EMIT>
__global__ void __launch_bounds__(kEdistRefBlock)
kmer_edist_hits_kernel(const uint8_t *__restrict__ data, unsigned long long n, unsigned lead, unsigned k, const u32x4 tab, unsigned tau,
                       unsigned *__restrict__ counts, unsigned *__restrict__ raw, const unsigned long long *__restrict__ tile_off,
                       unsigned long long *__restrict__ pos, uint8_t *__restrict__ hd, unsigned long long cap, unsigned long long pos_base,
                       unsigned long long *__restrict__ slot) {
    const unsigned long long nchunks = (n - lead + kEdistRefChunk - 1) / kEdistRefChunk;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEdistRefBlock;
    const unsigned long long ebase = pos_base + 1ull - lead; // end = (the column's index in the buffer) + ebase, modulo 2^64 in between
    for (unsigned long long c = (unsigned long long)blockIdx.x * kEdistRefBlock + threadIdx.x; c < nchunks; c += stride) {
        unsigned long long rank = 0;
        if constexpr (EMIT) {
            if (raw[c] == 0u) continue;
            rank = tile_off[c / kHitsTile] + counts[c];
            if (rank >= cap) continue;
        }
        const unsigned long long r0 = lead + c * kEdistRefChunk;
        const unsigned long long r1 = n - r0 < kEdistRefChunk ? n : r0 + kEdistRefChunk;
        const unsigned long long s = r0 >= kEdistRefLead ? r0 - kEdistRefLead : 0ull; // r0 < 64: the buffer's first chunk, a fresh column is its true initial column
        const uint32_t got = edist_hits_walk<PACKED, EMIT>(data, n, s, r0, r1, k, tab, tau, rank, ebase, pos, hd, cap, slot);
        if constexpr (!EMIT) counts[c] = got, raw[c] = got;
    }
}

} // namespace bitnuc_dev
