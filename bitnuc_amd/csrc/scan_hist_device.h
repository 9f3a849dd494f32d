// scan_hist_device.h -- the mismatch histogram per query in one pass: hist[q][d] = the number of windows j with
// hdist_scalar(as_2bit(ref[j .. j+k]), queries[q], k) == d (patterns: pdist), d < n_bins <= 16, on ASCII bytes (kmer_hist_kernel) and on packed 2-bit words
// (packed_hist_kernel).
//
// Skeleton and front end are the best match's (scan_best_device.h) unchanged: grid.y = query blocks of kMultiQB queries, kMultiBlock threads, the scan's
// tables (best_tables_kernel / BestTable) in the workgroup's LDS, one wave-private strip per wave, four MFMAs per 1024 windows, head and tail windows one per
// thread through QueryKind<Q>, invalid bytes latched by the first query block.  Only the back end is new.
//
// Binning.  Every A row carries the E8M0 scale 2^3 and the accumulators start at 2^23, so a result's bit pattern is 2^23 + 8 d and 2^23's low six bits are
// zero.  A TIER is one 64-bit register of eight 8-bit fields for eight consecutive distances.  Tier 0: y = min(x, 2^23 + 63), tier 1:
// y = med3(x, 2^23 + 63, 2^23 + 127); the low six bits of y -- all a 64-bit shift reads -- are 8 (d - 8 t) for a distance of the tier and 63 for every other,
// and (1 << 56) >> that is a one in field 7 - (d - 8 t), or ZERO: a window outside the tier is counted nowhere, so a tier has eight exact bins and no
// catch-all to correct.  One clamp, one 64-bit shift, one 64-bit add (v_lshl_add_u64): three vector instructions per window and tier.  n_bins <= 8 runs one
// tier, 9 - 16 two (the template parameter T, chosen by the launcher).
//
// Flushing.  A lane adds at most 64 windows per trip and query, so an 8-bit field holds three trips (192).  Every kHistPeriod trips and at the end a wave
// widens each register into four of two 16-bit fields (64 lanes x 192 = 12288), sums each over the wave (four DPP adds within a row of 16 lanes, the four
// rows through v_readlane), collects the sums of query qi in lane qi (a select) and lanes 0 - 15 add them into the workgroup's histogram in LDS
// (kMultiQB x 16 cells of 64 bits, 2 KiB).  The head and tail windows add into the same cells.  After a __syncthreads() one global atomicAdd per (workgroup,
// query, bin) with a non-zero count goes to hist[], which the launcher zeroes first in the same stream (graph-safe, no ticket; integer sums do not depend on
// the order of arrival: deterministic).  No global atomic per window, round or trip.
#pragma once
#include "device_prims.h"
#include "scan_best_device.h" // best_tables_kernel, best_tables_to_lds, BestTable; the front ends, query_operand and mfma_chain through it

namespace bitnuc_dev {

constexpr int kHistShift = 3;                  // A's row scale 2^3: a result is 2^23 + 8 d
constexpr int kHistScale = 127 + kHistShift;   // ... as an E8M0 exponent
constexpr int kHistMaxBins = 16;               // BITNUC_HIST_MAX_BINS: two tiers of eight
constexpr unsigned kHistPeriod = 3;            // trips between two flushes: 3 x 64 windows per lane and query fit an 8-bit field
constexpr uint32_t kHistBase = 0x4B000000u;    // 2^23 as a bit pattern
static_assert((kHistBase & 63u) == 0, "a 64-bit shift reads the low six bits of the clamped result");
static_assert(kHistPeriod * 64 <= 255 && kHistPeriod * 64 * 64 <= 65535, "a lane's 8-bit fields and a wave's 16-bit fields hold a flush period");

// where the accumulators start: 2^23 in all sixteen.  Sixteen registers used as an untied C operand (acc_start's note).
__device__ __forceinline__ f32x16 hist_acc_start() {
    f32x16 c0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c0[i] = bitnuc_host::kPackBias;
    asm volatile("" : "+v"(c0));
    return c0;
}

// a round's sixteen results into the lane's fields: tier t counts the distances 8 t .. 8 t + 7 (field 7 - (d - 8 t)) and nothing else
template <int T>
__device__ __forceinline__ void hist_bin_round(const f32x16 &acc, unsigned long long (&f)[T]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float v = acc[i]; // (__float_as_uint on a copy: pack_distances' note)
        const uint32_t x = __float_as_uint(v);
        f[0] += (1ull << 56) >> (min(x, kHistBase + 63u) & 63u);
        if constexpr (T > 1) f[1] += (1ull << 56) >> (min(max(x, kHistBase + 63u), kHistBase + 127u) & 63u);
    }
}

// Every query of the block against the trip in the strip: f[qi][t] += the lane's windows of the trip's m rounds.  read_b(u, B): round u's B operand.  The query
// loop is outside the round loop: a query's A operand is read once per trip (LDS order: lgkmcnt).
template <int U, int T, class ReadB>
__device__ __forceinline__ void hist_trip_queries(const BestTable *qtab, unsigned nq, unsigned row, unsigned m, const f32x16 &c0,
                                                  unsigned long long (&f)[kMultiQB][T], ReadB read_b) {
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) { // wave-uniform (a guard, not a break: the loop unrolls and f[][] stays in registers)
            i32x8 A[4];
            query_operand<4>(qtab[qi].w[row], A);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if ((unsigned)u >= m) break; // wave-uniform
                i32x8 B[4];
                read_b(u, B);
                hist_bin_round<T>(mfma_chain(A, B, c0, kHistScale), f[qi]);
            }
        }
    }
}

template <int CTRL> __device__ __forceinline__ uint32_t hist_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }

// the sum of v over the wave's 64 lanes (wave-uniform): quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror leave every lane of a row of
// sixteen with the row's sum; the four rows add on the scalar unit
__device__ __forceinline__ uint32_t hist_wave_sum(uint32_t v) {
    v += hist_dpp<0xB1>(v);
    v += hist_dpp<0x4E>(v);
    v += hist_dpp<0x141>(v);
    v += hist_dpp<0x140>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// The flush: the wave's fields into the workgroup's histogram, and zero.  wide[4 t + j] of lane qi collects query qi's sums: j = 0: fields 0 | 2 << 16,
// 1: fields 1 | 3, 2: fields 4 | 6, 3: fields 5 | 7 of tier t; field i of tier t is distance 8 t + 7 - i.
template <int T>
__device__ __forceinline__ void hist_flush(unsigned long long (&f)[kMultiQB][T], unsigned nq, unsigned lane, unsigned long long (*cells)[kHistMaxBins]) {
    uint32_t wide[4 * T];
#pragma unroll
    for (int j = 0; j < 4 * T; ++j) wide[j] = 0;
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint32_t lo = (uint32_t)f[qi][t], hi = (uint32_t)(f[qi][t] >> 32);
                const uint32_t part[4] = {lo & 0x00FF00FFu, (lo >> 8) & 0x00FF00FFu, hi & 0x00FF00FFu, (hi >> 8) & 0x00FF00FFu};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t sum = hist_wave_sum(part[j]);
                    wide[4 * t + j] = lane == (unsigned)qi ? sum : wide[4 * t + j];
                }
                f[qi][t] = 0;
            }
        }
    }
    if (lane < nq) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i0 = 4 * (j >> 1) + (j & 1); // the field in the low half; the high half is field i0 + 2
                const uint32_t a = wide[4 * t + j] & 0xFFFFu, b = wide[4 * t + j] >> 16;
                if (a) atomicAdd(&cells[lane][8 * t + 7 - i0], (unsigned long long)a);
                if (b) atomicAdd(&cells[lane][8 * t + 5 - i0], (unsigned long long)b);
            }
        }
    }
}

// The windows [0, pre) and [first, nwin), one per thread of the grid's x extent, every query of the block, into the workgroup's histogram: word_of(j) is
// window j's 2-bit word
template <class Q, class WordOf>
__device__ __forceinline__ void hist_tail_windows(unsigned long long pre, unsigned long long first, unsigned long long nwin, unsigned k,
                                                  const Q *__restrict__ queries, unsigned nq, unsigned long long (*cells)[kHistMaxBins], WordOf word_of) {
    const QueryKind<Q> kind(k);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (nwin > first ? nwin - first : 0);
    for (unsigned long long t = gt; t < total; t += nthreads) {
        const unsigned long long j = t < pre ? t : first + (t - pre);
        const auto w = kind.window(word_of(j));
#pragma unroll
        for (int qi = 0; qi < kMultiQB; ++qi) {
            if ((unsigned)qi < nq) {
                const uint32_t d = kind.dist(w, queries[qi]);
                if (d < (uint32_t)kHistMaxBins) atomicAdd(&cells[qi][d], 1ull);
            }
        }
    }
}

// the workgroup's histogram starts at zero (before best_tables_to_lds, whose barrier publishes it)
__device__ __forceinline__ void hist_cells_clear(unsigned long long (*cells)[kHistMaxBins]) {
    for (unsigned i = threadIdx.x; i < (unsigned)(kMultiQB * kHistMaxBins); i += blockDim.x) cells[i / kHistMaxBins][i % kHistMaxBins] = 0;
}

// The end: one atomicAdd per (query, bin < n_bins) of the workgroup with a non-zero count into hist[q * n_bins + d] (hist: the block's first query's row)
__device__ __forceinline__ void hist_reduce(unsigned long long (*cells)[kHistMaxBins], unsigned nq, unsigned n_bins, unsigned long long *__restrict__ hist) {
    __syncthreads();
    for (unsigned i = threadIdx.x; i < (unsigned)(kMultiQB * kHistMaxBins); i += blockDim.x) {
        const unsigned qi = i / kHistMaxBins, d = i % kHistMaxBins;
        if (qi < nq && d < n_bins) {
            const unsigned long long v = cells[qi][d];
            if (v) atomicAdd(hist + (size_t)qi * n_bins + d, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ASCII bytes at any alignment: the rounds start at ref + skip (16-byte aligned).
template <int U, int T, class Q>
__global__ void __launch_bounds__(kMultiBlock)
kmer_hist_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries, unsigned n_queries,
                 unsigned n_bins, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ hist, unsigned long long *__restrict__ slot) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][AsciiStrip4<U>::kBytes];
    __shared__ unsigned long long cells[kMultiQB][kHistMaxBins];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    const bool latch = blockIdx.y == 0; // one query block reports invalid bytes
    hist_cells_clear(cells);
    best_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = ref + skip;
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const AsciiStrip4<U> fe(strips[wave_in_block()], lane);
    unsigned long long f[kMultiQB][T];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi)
#pragma unroll
        for (int t = 0; t < T; ++t) f[qi][t] = 0;

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
    const f32x16 c0 = hist_acc_start();

    unsigned held = 0; // trips in f[][] since the last flush
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
        hist_trip_queries<U, T>(qtab, nq, fe.row, m, c0, f, [&](int u, i32x8 (&B)[4]) { fe.read_b(u, B); });
        r0 = rn;
        if (++held == kHistPeriod) { // wave-uniform
            hist_flush<T>(f, nq, lane, cells);
            held = 0;
        }
    }
    if (held) hist_flush<T>(f, nq, lane, cells);

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    hist_tail_windows(pre, first, nwin, k, queries + q0, nq, cells, [&](unsigned long long j) { return ascii_window_word(ref, j, k, latch, slot); });
    hist_reduce(cells, nq, n_bins, hist + (size_t)q0 * n_bins);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed words (8-byte aligned; at 8 mod 16 the rounds start one word later).
template <int T, class Q>
__global__ void __launch_bounds__(kMultiBlock)
packed_hist_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries, unsigned n_queries,
                   unsigned n_bins, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ hist) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][PackedStrip4::kBytes];
    __shared__ unsigned long long cells[kMultiQB][kHistMaxBins];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    hist_cells_clear(cells);
    best_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    uint8_t *strip = strips[wave_in_block()];
    const PackedStrip4 fe(strip, lane);
    unsigned rd[4]; // (here and not in fe: read_offsets' note)
    fe.read_offsets(rd);
    unsigned long long f[kMultiQB][T];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi)
#pragma unroll
        for (int t = 0; t < T; ++t) f[qi][t] = 0;

    unsigned long long r0 = wave * 4;
    PackedTrip cur;
    if (r0 < rounds) packed_trip_load(base, r0, rounds, lane, cur);
    const f32x16 c0 = hist_acc_start();

    unsigned held = 0;
    while (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, 4u);
        const unsigned long long rn = r0 + nwaves * 4;
        wave_lds_fence(); // the previous trip's readers are done
        fe.fill(lane, m, cur);
        if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
        wave_lds_fence();
        hist_trip_queries<4, T>(qtab, nq, fe.row, m, c0, f, [&](int u, i32x8 (&B)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) B[j] = PackedStrip4::operand(strip, rd[j], u);
        });
        r0 = rn;
        if (++held == kHistPeriod) {
            hist_flush<T>(f, nq, lane, cells);
            held = 0;
        }
    }
    if (held) hist_flush<T>(f, nq, lane, cells);

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    hist_tail_windows(pre, first, nwin, k, queries + q0, nq, cells, [&](unsigned long long j) { return packed_window_word(words, j, k); });
    hist_reduce(cells, nq, n_bins, hist + (size_t)q0 * n_bins);
}

} // namespace bitnuc_dev
