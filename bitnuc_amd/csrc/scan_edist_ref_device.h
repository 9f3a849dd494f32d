// scan_edist_ref_device.h -- the INDEL-TOLERANT k-mer search ALONG A REFERENCE (bitnuc_kmer_edist_best*, bitnuc_kmer_edist_count_multi* and their
// bitnuc_kmer_pattern_edist_* twins): with E_q(j) = D[k][j] the edit distance of query q to the best substring of the reference that ends at base j
// (D[0][j] = 0, D[i][0] = i: the substring starts anywhere and may be empty; `end` j is one past the last aligned base, 1 <= j <= n),
//   best:   dist[q] = min over j of E_q(j), end[q] = the smallest j that attains it;
//   count:  counts[q] = #{ j : E_q(j) <= taus[q] }.
// This is scan_edist_device.h's distance with the whole reference as the span; the step is the same bit-parallel recurrence (Myers 1999 in Hyyro's
// form: a column in Pv / Mv, one 32-bit add per base, bit k - 1 of Ph / Mh moves the score): edist_step_device.h's, shared with the per-read kernels
// and the hit list; the loops around it are this file's.  A vector-ALU kernel: the recurrence is a carry chain, not a contraction.
//
// CHUNKS.  The recurrence is sequential along the reference, so the end positions are cut into chunks of kEdistRefChunk = 1024 columns, ONE CHUNK PER
// LANE.  The lane that owns the (0-based) columns [r0, r1) starts a FRESH column (Pv = ~0, Mv = 0, score = k) kEdistRefLead = 64 columns earlier, at
// s = r0 - 64, and reports nothing of the lead-in.  That is exact: a fresh start before column s computes the minimum over the substrings that start at
// or after s; an optimal substring that ends at j has at most 2k bases (a longer one costs more than k, which the empty substring costs), so from column
// s + 2k on the fresh value IS E(j).  64 = 2 * 32 >= 2k for every k and keeps the first reported column on a trip boundary for every
// k; the chunk at the start of the buffer has no lead-in, its fresh column is the true initial column.  Cost: (1024 + 64) / 1024 steps per column.
// `lead` (the internal launch argument of the host chunk loops): the first `lead` <= 64 columns of the buffer are run but not reported -- they are the
// tail of the previous host chunk, which reported them.  Every column is reported by exactly one lane of exactly one launch.
//
// TRIPS.  A lane streams its chunk 64 codes at a time into four registers of 2-bit codes: packed words as 16 bytes, ASCII as four unaligned 16-byte
// loads (any byte alignment) through dword_residue / enc4, an invalid byte found by rescan_bytes and latched by atomicMin (the first in sequence order
// wins, however many lanes see it).  The last trip of the buffer loads only bytes / words that hold a base of it.  The next trip's loads are issued
// before the current trip's steps.  A trip whose 64 columns are all reported runs the FAST steps; the others (the lead-in, the first trip behind a
// `lead` that is no multiple of 64, the last trip of the buffer) run the general ones, whose per-step range test is paid once for all interleaved queries.
//
// QUERIES.  kEdistInterleave queries run side by side through one walk over the chunk (remainders of Q as groups of 2 and 1; the loop is wave-uniform),
// and the chunk is walked again for each group while it is still in the caches.  Tables: edist_tables_kernel's 16 bytes per query, one form for exact
// queries and patterns, so there is one main kernel for both kinds.  Eq is two levels of selects on the base's two code bits.
//
// RESULTS.  Best: per step one v_min of (score << 11 | the step's index in the walk < 2048); per (chunk, query) the 64-bit key score << 58 | end, the
// wave's minimum by shuffles and one atomicMin per (wave, query, chunk round) that saw a reported column, into the per-query keys in context scratch
// (all-ones first, in stream order); edist_ref_finish_kernel writes end[] / dist[].  Count: a per-lane counter of reported columns with score <= tau, the
// wave's sum, one atomicAdd per (wave, query, chunk round) with a non-zero sum into counts[] (zeroed first).  Minimum and sum do not depend on the
// order of arrival: deterministic, graph-safe, no ticket, no LDS.  All position arithmetic is 64-bit (chunk index * 1024, s, the key's end field).
// The grid is bounded (kEdistRefBlocksPerCu workgroups per CU); a lane walks chunks at the grid's stride: 2^29 bases per round of a 256-CU device.
#pragma once
#include "device_prims.h"
#include "edist_step_device.h" // EdistCols, edist_cols_init, edist_eq, edist_step
#include "scan_edist_device.h" // edist_tables_kernel
#include "scan_mfma_device.h"  // dword_residue, trip_invalid

namespace bitnuc_dev {

constexpr unsigned kEdistRefChunk = 1024;       // C: reported columns per lane and chunk round (tests/test_gpu_kmer_edist.py repeats it)
constexpr unsigned kEdistRefLead = 64;          // columns a lane runs in front of its chunk without reporting them: >= 2k for every k <= 32
constexpr unsigned kEdistRefTrip = 64;          // columns per trip: four registers of sixteen 2-bit codes
constexpr int kEdistRefBlock = 256;             // four waves, nothing shared between them
constexpr unsigned kEdistRefBlocksPerCu = 8;    // the grid's bound
constexpr unsigned kEdistRefStepBits = 11;      // a step's index in the walk: < kEdistRefChunk + 2 kEdistRefLead <= 2048
constexpr int kEdistRefEndBits = 58;            // key = dist << 58 | end, as the Hamming best match's
static_assert(kEdistRefChunk % kEdistRefTrip == 0 && kEdistRefLead % kEdistRefTrip == 0, "the first reported column of a chunk starts a trip");
static_assert(kEdistRefChunk + 2 * kEdistRefLead <= (1u << kEdistRefStepBits), "the step index fits the lane's key");

// ---- a trip's 64 codes.  b: the trip's first column, b < n; only bytes / words that hold a column < n are loaded
struct EdistRefRawAscii { u32x4 v[4]; };
__device__ __forceinline__ EdistRefRawAscii edist_ref_load_ascii(const uint8_t *__restrict__ ref, unsigned long long b, unsigned long long n) {
    EdistRefRawAscii r;
    const unsigned long long left = n - b;
    if (left >= kEdistRefTrip) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r.v[i] = *reinterpret_cast<const u32x4_u *>(ref + b + 16 * i);
    } else { // the buffer's last trip: byte by byte, 'A' behind the last base
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t x = 0x41414141u;
#pragma unroll
                for (unsigned e = 0; e < 4; ++e) {
                    const unsigned at = 16u * i + 4u * d + e;
                    if (at < left) x = (x & ~(0xFFu << (8u * e))) | ((uint32_t)ref[b + at] << (8u * e));
                }
                r.v[i][d] = x;
            }
        }
    }
    return r;
}
template <bool VALIDATE = true>
__device__ __forceinline__ void edist_ref_codes(const EdistRefRawAscii &r, const uint8_t *__restrict__ ref, unsigned long long b, unsigned long long n,
                                                unsigned long long *__restrict__ slot, uint32_t (&codes)[4]) {
    uint32_t bad = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t c = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t x = r.v[w][e];
            if constexpr (VALIDATE) bad |= dword_residue(x);
            uint32_t unused = 0;
            c |= enc4(x, unused) << (8 * e);
        }
        codes[w] = c;
    }
    if (VALIDATE && __builtin_expect(trip_invalid(bad), 0)) rescan_bytes(ref, b, n - b < kEdistRefTrip ? (unsigned)(n - b) : kEdistRefTrip, slot);
}

struct EdistRefRawPacked { unsigned long long w0, w1; };
// b is a multiple of 32 (the chunks, the lead-in and a packed `lead` all are); bits above 2n of the last word are junk behind the last reported column
__device__ __forceinline__ EdistRefRawPacked edist_ref_load_packed(const uint64_t *__restrict__ words, unsigned long long b, unsigned long long n) {
    const unsigned long long *p = reinterpret_cast<const unsigned long long *>(words) + (b >> 5);
    EdistRefRawPacked r;
    r.w0 = p[0];
    r.w1 = n - b > 32ull ? p[1] : 0ull;
    return r;
}
template <bool VALIDATE = true>
__device__ __forceinline__ void edist_ref_codes(const EdistRefRawPacked &r, const uint8_t *, unsigned long long, unsigned long long, unsigned long long *,
                                                uint32_t (&codes)[4]) {
    codes[0] = (uint32_t)r.w0, codes[1] = (uint32_t)(r.w0 >> 32), codes[2] = (uint32_t)r.w1, codes[3] = (uint32_t)(r.w1 >> 32);
}

template <bool PACKED> struct EdistRefRaw { using type = EdistRefRawAscii; };
template <> struct EdistRefRaw<true> { using type = EdistRefRawPacked; };
template <bool PACKED>
__device__ __forceinline__ typename EdistRefRaw<PACKED>::type edist_ref_load(const uint8_t *__restrict__ data, unsigned long long b, unsigned long long n) {
    if constexpr (PACKED) return edist_ref_load_packed(reinterpret_cast<const uint64_t *>(data), b, n);
    else return edist_ref_load_ascii(data, b, n);
}

// U queries' columns and results of one lane.  acc: best: the smallest (score << kEdistRefStepBits | step) over the reported columns; count: the
// reported columns with score <= tau
template <int U> struct EdistRefState : EdistCols<U> { uint32_t acc[U], tau[U]; };

// the 64 steps of a trip.  t0: the walk index of the trip's first step (wave-uniform).  FAST: every column is reported; otherwise those with
// lo <= (index in the trip) < lo + width, per lane
template <int U, bool COUNT, bool FAST>
__device__ __forceinline__ void edist_ref_steps(const uint32_t (&codes)[4], unsigned top, EdistRefState<U> &st, unsigned t0, unsigned lo, unsigned width) {
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        uint32_t c = codes[w];
#pragma unroll 1
        for (unsigned s = 0; s < 16; ++s) {
            const uint32_t lowm = 0u - (c & 1u); // the base's low code bit as a mask
            const bool hi = (c & 2u) != 0u;
            c >>= 2;
            const unsigned tl = 16u * w + s;
            uint32_t off = 0u; // all-ones at a column that is not reported: once per step, not per query
            if constexpr (!FAST) off = (tl - lo) < width ? 0u : ~0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (COUNT) {
                    // spelled here: through edist_step, in any of the forms tried, kmer_edist_kernel<packed, count> compiles to another order of its step loops
                    // and measures 1 - 2 % slower
                    const uint32_t eq = edist_eq(st, u, lowm, hi);
                    const uint32_t xv = eq | st.mv[u];
                    const uint32_t xh = (((eq & st.pv[u]) + st.pv[u]) ^ st.pv[u]) | eq;
                    uint32_t ph = st.mv[u] | ~(xh | st.pv[u]);
                    uint32_t mh = st.pv[u] & xh;
                    st.sc[u] += (ph >> top) & 1u;
                    st.sc[u] -= (mh >> top) & 1u;
                    const uint32_t hit = st.sc[u] <= st.tau[u] ? 1u : 0u;
                    st.acc[u] += FAST ? hit : (hit & ~off);
                    ph <<= 1; // no carry-in: D[0][j] = 0
                    mh <<= 1;
                    st.pv[u] = mh | ~(xv | ph);
                    st.mv[u] = ph & xv;
                } else {
                    edist_step(st, u, edist_eq(st, u, lowm, hi), top,
                               [&](uint32_t sc) { st.acc[u] = min(st.acc[u], ((sc << kEdistRefStepBits) + (t0 + tl)) | off); });
                }
            }
        }
    }
}

// queries q0 .. q0 + U - 1 along the lane's walk: columns [s, r1) of which [r0, r1) are reported; units == 0: a lane without a chunk (it still takes
// part in the wave's reduction).  out: the per-query keys (best) or counts (count)
template <bool PACKED, bool COUNT, int U>
__device__ __forceinline__ void edist_ref_queries(const uint8_t *__restrict__ data, unsigned long long n, unsigned long long s, unsigned long long r0,
                                                  unsigned long long r1, unsigned units, unsigned k, const u32x4 *__restrict__ tabs,
                                                  const uint32_t *__restrict__ taus, unsigned q0, unsigned long long *__restrict__ out,
                                                  unsigned long long *__restrict__ slot) {
    EdistRefState<U> st;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        edist_cols_init(st, u, tabs[q0 + u], k);
        st.acc[u] = COUNT ? 0u : ~0u;
        st.tau[u] = 0u;
        if constexpr (COUNT) st.tau[u] = taus[q0 + u];
    }
    const unsigned top = k - 1u;
    if (units) {
        auto raw = edist_ref_load<PACKED>(data, s, n);
        for (unsigned u = 0; u < units; ++u) {
            const unsigned long long b = s + (unsigned long long)u * kEdistRefTrip;
            uint32_t codes[4];
            edist_ref_codes(raw, data, b, n, slot, codes);
            if (u + 1u < units) raw = edist_ref_load<PACKED>(data, b + kEdistRefTrip, n); // b + 64 < r1 <= n
            if (b >= r0 && b + kEdistRefTrip <= r1) {
                edist_ref_steps<U, COUNT, true>(codes, top, st, u * kEdistRefTrip, 0u, 0u);
            } else {
                const unsigned lo = r0 > b ? (r0 - b < kEdistRefTrip ? (unsigned)(r0 - b) : kEdistRefTrip) : 0u;
                const unsigned hi = r1 - b < kEdistRefTrip ? (unsigned)(r1 - b) : kEdistRefTrip; // r1 > b
                edist_ref_steps<U, COUNT, false>(codes, top, st, u * kEdistRefTrip, lo, hi - lo);
            }
        }
    }
    const unsigned lane = threadIdx.x & 63u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (COUNT) {
            uint32_t v = st.acc[u];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0 && v) atomicAdd(out + q0 + u, (unsigned long long)v);
        } else {
            const uint32_t a = st.acc[u];
            unsigned long long v = a == ~0u ? ~0ull
                                            : ((unsigned long long)(a >> kEdistRefStepBits) << kEdistRefEndBits) |
                                                  (s + (a & ((1u << kEdistRefStepBits) - 1u)) + 1ull);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(v, off);
                v = o < v ? o : v;
            }
            if (lane == 0 && v != ~0ull) atomicMin(out + q0 + u, v);
        }
    }
}

// data: n >= 1 bases (ASCII bytes at any alignment, or 8-byte aligned packed words); lead < n columns are run but not reported, lead <= kEdistRefLead
// and, packed, a multiple of 32; 1 <= k <= 32; 1 <= nq; tabs: nq entries of edist_tables_kernel; taus: nq thresholds (count only).  out: nq keys set to
// all-ones (best) or nq counts set to zero (count).  blockDim.x == kEdistRefBlock; any grid: chunks are walked at the grid's stride.
template <bool PACKED, bool COUNT>
__global__ void __launch_bounds__(kEdistRefBlock)
kmer_edist_kernel(const uint8_t *__restrict__ data, unsigned long long n, unsigned lead, unsigned k, unsigned nq, const u32x4 *__restrict__ tabs,
                  const uint32_t *__restrict__ taus, unsigned long long *__restrict__ out, unsigned long long *__restrict__ slot) {
    const unsigned long long nchunks = (n - lead + kEdistRefChunk - 1) / kEdistRefChunk;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEdistRefBlock;
    const unsigned lane = threadIdx.x & 63u;
    // the wave's first chunk decides the trip: every lane of a wave that has a chunk stays for the shuffles
    for (unsigned long long cw = (unsigned long long)blockIdx.x * kEdistRefBlock + (threadIdx.x & ~63u); cw < nchunks; cw += stride) {
        const unsigned long long c = cw + lane;
        unsigned long long s = 0, r0 = 0, r1 = 0;
        unsigned units = 0;
        if (c < nchunks) {
            r0 = lead + c * kEdistRefChunk;
            r1 = n - r0 < kEdistRefChunk ? n : r0 + kEdistRefChunk;
            s = r0 >= kEdistRefLead ? r0 - kEdistRefLead : 0ull; // r0 < 64: the buffer's first chunk, a fresh column is its true initial column
            units = (unsigned)((r1 - s + kEdistRefTrip - 1) / kEdistRefTrip);
        }
        unsigned q = 0;
#pragma unroll 1
        for (; q + kEdistInterleave <= nq; q += kEdistInterleave) edist_ref_queries<PACKED, COUNT, kEdistInterleave>(data, n, s, r0, r1, units, k, tabs, taus, q, out, slot);
        if (nq - q >= 2u) { edist_ref_queries<PACKED, COUNT, 2>(data, n, s, r0, r1, units, k, tabs, taus, q, out, slot); q += 2u; }
        if (nq - q >= 1u) edist_ref_queries<PACKED, COUNT, 1>(data, n, s, r0, r1, units, k, tabs, taus, q, out, slot);
    }
}

// keys[q] -> end[q], dist[q] (dist at any byte offset); `sub` is taken from every end (the host chunk loops: the buffer's lead-in)
__global__ void __launch_bounds__(256) edist_ref_finish_kernel(const unsigned long long *__restrict__ keys, unsigned n_queries, unsigned long long sub,
                                                               unsigned long long *__restrict__ end, uint8_t *__restrict__ dist) {
    const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    const unsigned long long key = keys[q];
    const bool none = key == ~0ull;
    end[q] = none ? ~0ull : (key & ((1ull << kEdistRefEndBits) - 1)) - sub;
    dist[q] = none ? (uint8_t)0xFF : (uint8_t)(key >> kEdistRefEndBits);
}

} // namespace bitnuc_dev
