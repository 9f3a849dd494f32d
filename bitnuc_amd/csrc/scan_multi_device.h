// scan_multi_device.h -- the fused k-mer count for MANY queries in one pass: counts[q] = the number of windows j with
// hdist_scalar(as_2bit(ref[j .. j+k]), queries[q], k) <= taus[q], on ASCII bytes (kmer_count3_multi_kernel) and on packed 2-bit words
// (packed_count3_multi_kernel).
//
// The contraction is the three-channel count's (scan_mfma_device.h): a column is a segment of 32 consecutive windows, a row one of its
// 32 shifts, three MFMAs per 1024 windows, the d <= tau test inside the product.  The reference's side of the product (B, the one-hot strip) does not
// depend on the query; only the query's table (A) and the accumulator's start values do.  So a wave writes a trip's strip ONCE and runs every query of
// its block against it:
//   * grid.y = query blocks of kMultiQB queries; each lane keeps one hit counter per query of its block in registers, so nothing is reduced until the end;
//   * the block's tables (Count3MfmaTable: 3 KiB + the start values per query) are copied into the workgroup's LDS once; a query's A operand and start
//     values are ds_reads per trip, in LDS order (lgkmcnt), so they never wait behind the next trip's global loads (query_operand's vmcnt(0) trap);
//   * per query and round: the three ds_read_b128 of B (as the single count), three MFMAs, hit_bits + v_bcnt into the query's counter;
//   * front end: AsciiStrip3 (scan_mfma_device.h) and PackedStrip3 (scan_packed_device.h); invalid-byte rule and next-trip prefetch as the single counts;
//   * the end: one wave reduction per query, the waves' sums through LDS, one 64-bit atomic add per (workgroup, query) into counts[] -- which the
//     launcher zeroes first in the same stream (graph-safe, no ticket).
// The tables are built in-stream by count3_tables_kernel from the queries and thresholds in device memory, with the host's builder (scan_mfma_host.h:
// count3_mfma_lane / count3_packed_lane, one thread per lane) into context scratch.
//
// Windows the rounds do not cover: ASCII input at any alignment starts its rounds at the first 16-byte aligned base (skip = (-ref) mod 16, the hit
// lists' rule), packed words at 8 mod 16 one word later (skip = 32); the windows [0, skip) and those after the last whole round go to the grid's
// threads one window each, every query of the block per window.  Invalid bytes are latched by the first query block only (the slot keeps the first
// invalid byte of the sequence: one latch per call, whatever the number of queries).
#pragma once
#include "device_prims.h"
#include "scan_mfma_device.h"   // the front end: scan_trip_load, AsciiStrip3; the back end: query_operand, acc_start, count_row_scale, mfma_chain, hit_bits
#include "scan_packed_device.h" // the packed front end: packed_trip_load, PackedStrip3
#include "scan_mfma_host.h"     // Count3Rule, count3_mfma_lane, count3_packed_lane

namespace bitnuc_dev {

constexpr int kMultiQB = 16;     // queries per workgroup (grid.y block): one per-lane counter each
constexpr int kMultiBlock = 768; // threads per workgroup: 12 waves, one workgroup per CU (its LDS: 16 tables + 12 strips)
constexpr int kMultiRounds = 4;  // rounds per trip (ASCII; a packed trip is one 1 KiB wave load = 4 rounds)
static_assert(sizeof(Count3MfmaTable) % 16 == 0, "tables are copied and read as 16-byte pieces");
using bitnuc_host::Count3Rule;

// One thread per (query, lane): lane's 12 dwords of query q's table, lane 0 also its start values.  Q: the query kind (QueryKind, scan_mfma_device.h) --
// Count3Rule takes either
template <bool PACKED, class Q>
__global__ void __launch_bounds__(64) count3_tables_kernel(const Q *__restrict__ queries, const unsigned *__restrict__ taus, unsigned k,
                                                           Count3MfmaTable *__restrict__ tabs) {
    const unsigned q = blockIdx.x, lane = threadIdx.x;
    const Count3Rule r(queries[q], k, taus[q], false);
    if constexpr (PACKED) bitnuc_host::count3_packed_lane(r, (int)lane, tabs[q].w[lane]);
    else bitnuc_host::count3_mfma_lane(r, (int)lane, tabs[q].w[lane]);
    if (lane == 0) r.start(tabs[q].c);
}

// the block's nq tables -> LDS (whole workgroup, before anything reads them)
__device__ __forceinline__ void multi_tables_to_lds(const Count3MfmaTable *__restrict__ tabs, unsigned nq, Count3MfmaTable *lds) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(tabs);
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
    const unsigned nv = nq * (unsigned)(sizeof(Count3MfmaTable) / 16);
    for (unsigned i = threadIdx.x; i < nv; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// Every query of the block against the trip in the strip (fe: its front end): hits[qi] += the windows of the trip's m rounds with d <= tau_qi (lane's
// share).  The query loop is outside the round loop: a query's A operand and start values are read once per trip.
template <int U, class Front>
__device__ __forceinline__ void multi_trip_queries(const Count3MfmaTable *qtab, unsigned nq, unsigned lane, unsigned m, int scale_a, uint32_t (&hits)[kMultiQB],
                                                   const Front &fe) {
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) { // wave-uniform (a guard, not a break: the loop unrolls and hits[] stays in registers)
            i32x8 A[3];
            query_operand<3>(qtab[qi].w[lane], A);
            const f32x16 c0 = acc_start(qtab[qi].c);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if ((unsigned)u >= m) break; // wave-uniform
                i32x8 B[3];
                fe.read_b(u, B);
                const f32x16 acc = mfma_chain(A, B, c0, scale_a);
#pragma unroll
                for (int q = 0; q < 4; ++q) hits[qi] += (uint32_t)__builtin_popcount(hit_bits(acc, q));
            }
        }
    }
}

// The windows [0, pre) and [first, nwin), one per thread of the grid's x extent, every query of the block: word_of(j) is window j's 2-bit word
template <class Q, class WordOf>
__device__ __forceinline__ void multi_tail_windows(unsigned long long pre, unsigned long long first, unsigned long long nwin, unsigned k,
                                                   const Q *__restrict__ queries, const unsigned *__restrict__ taus, unsigned nq,
                                                   uint32_t (&hits)[kMultiQB], WordOf word_of) {
    const QueryKind<Q> kind(k);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (nwin > first ? nwin - first : 0);
    for (unsigned long long t = gt; t < total; t += nthreads) {
        const unsigned long long j = t < pre ? t : first + (t - pre);
        const auto w = kind.window(word_of(j));
#pragma unroll
        for (int qi = 0; qi < kMultiQB; ++qi) {
            if ((unsigned)qi < nq) hits[qi] += kind.dist(w, queries[qi]) <= taus[qi] ? 1u : 0u;
        }
    }
}

// The end: per query, the wave's sum, the workgroup's through LDS, one atomic add per (workgroup, query) that found a hit
__device__ __forceinline__ void multi_reduce(uint32_t (&hits)[kMultiQB], unsigned nq, unsigned lane, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t part[kMultiBlock / 64][kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) {
            uint32_t h = hits[qi];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
            if (lane == 0) part[threadIdx.x >> 6][qi] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < nq) {
        unsigned long long s = 0;
        for (unsigned w = 0; w < (blockDim.x >> 6); ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(counts + threadIdx.x, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ASCII bytes at any alignment: the rounds start at ref + skip (16-byte aligned).
template <int U, class Q>
__global__ void __launch_bounds__(kMultiBlock)
kmer_count3_multi_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries,
                         const unsigned *__restrict__ taus, unsigned n_queries, const Count3MfmaTable *__restrict__ tabs,
                         unsigned long long *__restrict__ counts, unsigned long long *__restrict__ slot) {
    __shared__ __attribute__((aligned(16))) Count3MfmaTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][AsciiStrip3<U>::kBytes];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    const bool latch = blockIdx.y == 0; // one query block reports invalid bytes
    multi_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = ref + skip;
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const AsciiStrip3<U> fe(strips[wave_in_block()], lane);
    uint32_t hits[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) hits[qi] = 0;

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
    const int scale_a = count_row_scale(lane & 31u);

    while (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, U);
        const unsigned long long rn = r0 + nwaves * U;
        wave_lds_fence(); // the previous trip's readers are done
        const uint32_t trip_bad = fe.fill(lane, m, cur);
        if (latch && __builtin_expect(trip_invalid(trip_bad), 0)) {
#pragma unroll 1
            for (unsigned u = 0; u < m; ++u) rescan_bytes(ref, skip + ((r0 + u) << 10) + 16 * lane, 16, slot);
        }
        if (rn < rounds) scan_trip_load<U, 3, true>(base, rn, rounds, lane, cur); // cur's bytes are in the strip: its registers take the next trip
        wave_lds_fence();
        multi_trip_queries<U>(qtab, nq, lane, m, scale_a, hits, fe);
        r0 = rn;
    }

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    multi_tail_windows(pre, first, nwin, k, queries + q0, taus + q0, nq, hits, [&](unsigned long long j) { return ascii_window_word(ref, j, k, latch, slot); });
    multi_reduce(hits, nq, lane, counts + q0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed words (8-byte aligned; at 8 mod 16 the rounds start one word later).
template <class Q>
__global__ void __launch_bounds__(kMultiBlock)
packed_count3_multi_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries,
                           const unsigned *__restrict__ taus, unsigned n_queries, const Count3MfmaTable *__restrict__ tabs,
                           unsigned long long *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) Count3MfmaTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][PackedStrip3::kBytes];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    multi_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const PackedStrip3 fe(strips[wave_in_block()], lane);
    uint32_t hits[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) hits[qi] = 0;

    unsigned long long r0 = wave * 4;
    PackedTrip cur;
    if (r0 < rounds) packed_trip_load(base, r0, rounds, lane, cur);
    const int scale_a = count_row_scale(lane & 31u);

    while (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, 4u);
        const unsigned long long rn = r0 + nwaves * 4;
        wave_lds_fence(); // the previous trip's readers are done
        fe.fill(lane, m, cur);
        if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
        wave_lds_fence();
        multi_trip_queries<4>(qtab, nq, lane, m, scale_a, hits, fe);
        r0 = rn;
    }

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    multi_tail_windows(pre, first, nwin, k, queries + q0, taus + q0, nq, hits, [&](unsigned long long j) { return packed_window_word(words, j, k); });
    multi_reduce(hits, nq, lane, counts + q0);
}

} // namespace bitnuc_dev
