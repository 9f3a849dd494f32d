// scan_best_device.h -- the best match per query in one pass: dist[q] = min over the windows j of hdist_scalar(as_2bit(ref[j .. j+k]), queries[q], k),
// pos[q] = the smallest j that attains it, on ASCII bytes (kmer_best_kernel) and on packed 2-bit words (packed_best_kernel).
//
// The skeleton is the multi-query count's (scan_multi_device.h): grid.y = query blocks of kMultiQB queries, kMultiBlock threads, the block's tables in the
// workgroup's LDS, one wave-private strip per wave written once per trip, every query of the block run against it, head and tail windows one per thread.
// The count's 6-bit threshold fields carry no distance, so the contraction is the scan's: FOUR channels per base (AsciiStrip4 / PackedStrip4, four MFMAs
// per 1024 windows) and the scan's query tables, one row per thread built in-stream by best_tables_kernel (scan_mfma_host.h: scan_seg_row,
// scan_packed_row) into context scratch.
//
// The running minimum lives in the accumulator.  Every A row carries the E8M0 scale 2^4 and result register r starts at 2^23 + r, so a result is the
// integer 2^23 + 16 d + r (d <= 32: exact below 2^24) and, all sixteen having one exponent, their bit patterns order like (d, r).  A lane's registers
// cover its windows in ascending order (lane (n, h), register r: window 32 n + 8 (r >> 2) + 4 h + (r & 3) of the round), so an unsigned minimum over the
// sixteen (eight v_min3_u32 / v_min_u32) is the lane's smallest distance and the FIRST register that holds it.  (key | 15) < best says d < the best d: one
// v_or, one compare and two selects keep (key, the wave's round counter) on a strict improvement only -- a wave walks its trips in ascending order, so the
// leftmost window of a lane survives.  Twelve vector instructions per round and query, as the count; nothing on the scalar unit.
//
// The end: each lane turns (key, round counter) into the 64-bit key d << 58 | j (all position arithmetic in 64 bits), the head and tail windows feed the
// same per-lane keys, a wave reduction and the waves' minima through LDS leave one atomicMin per (workgroup, query) into keys[] -- which the launcher sets
// to all-ones first in the same stream (graph-safe, no ticket; a minimum does not depend on the order of arrival: deterministic).  best_finish_kernel
// writes pos[q] / dist[q]; the all-ones key (no window) gives UINT64_MAX / 0xFF.
// Invalid bytes (ASCII) are latched by the first query block only, as kmer_count3_multi_kernel does.
#pragma once
#include "device_prims.h"
#include "scan_mfma_device.h"   // the front end: scan_trip_load, AsciiStrip4; the back end: query_operand, mfma_chain
#include "scan_packed_device.h" // the packed front end: packed_trip_load, PackedStrip4
#include "scan_multi_device.h"  // kMultiQB, kMultiBlock, kMultiRounds
#include "scan_mfma_host.h"     // BestTable, scan_seg_row, scan_packed_row

namespace bitnuc_dev {

constexpr int kBestShift = 4;                        // A's row scale 2^4: a result is 2^23 + 16 d + r
constexpr int kBestScale = 127 + kBestShift;         // ... as an E8M0 exponent
constexpr uint32_t kBestNone = 0xFFFFFFFFu;          // a lane that has seen no round
constexpr unsigned long long kBestNoKey = ~0ull;     // a query that has seen no window
constexpr int kBestPosBits = 58;                     // key = d << 58 | j
static_assert(sizeof(BestTable) % 16 == 0, "tables are copied and read as 16-byte pieces");

// One thread per (query, row): row's 16 dwords of query q's table (ASCII: delta = row - 8, 40 rows; packed: delta = row - 2, 34 rows)
// Q: the query kind (QueryKind, scan_mfma_device.h) -- the row builders take either
template <bool PACKED, class Q>
__global__ void __launch_bounds__(64) best_tables_kernel(const Q *__restrict__ queries, unsigned k, BestTable *__restrict__ tabs) {
    const unsigned q = blockIdx.x, row = threadIdx.x;
    if constexpr (PACKED) {
        if (row < 34u) bitnuc_host::scan_packed_row(queries[q], k, (int)row - 2, tabs[q].w[row]);
    } else {
        if (row < (unsigned)kBestRows) bitnuc_host::scan_seg_row(queries[q], k, (int)row - 8, tabs[q].w[row]);
    }
}

// the block's nq tables -> LDS (whole workgroup, before anything reads them)
__device__ __forceinline__ void best_tables_to_lds(const BestTable *__restrict__ tabs, unsigned nq, BestTable *lds) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(tabs);
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
    const unsigned nv = nq * (unsigned)(sizeof(BestTable) / 16);
    for (unsigned i = threadIdx.x; i < nv; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// where the accumulators start: result register r at 2^23 + r.  Sixteen registers used as an untied C operand (acc_start's note).
__device__ __forceinline__ f32x16 best_acc_start() {
    f32x16 c0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c0[i] = bitnuc_host::kPackBias + (float)i;
    asm volatile("" : "+v"(c0));
    return c0;
}

// the smallest of a round's sixteen results as bit patterns: 2^23 + 16 d + r of the lane's first window with its smallest d
__device__ __forceinline__ uint32_t round_min_key(const f32x16 &acc) {
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float f = acc[i]; // (__float_as_uint on a copy: pack_distances' note)
        x[i] = __float_as_uint(f);
    }
    uint32_t m = min(min(x[0], x[1]), x[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) m = min(min(m, x[i]), x[i + 1]);
    return min(m, x[15]);
}

// Every query of the block against the trip in the strip: (best[qi], at[qi]) = the lane's smallest key so far and the round counter t0 + u it was met at.
// read_b(u, B): round u's B operand.  The query loop is outside the round loop: a query's A operand is read once per trip (LDS order: lgkmcnt).
template <int U, class ReadB>
__device__ __forceinline__ void best_trip_queries(const BestTable *qtab, unsigned nq, unsigned row, unsigned m, const f32x16 &c0, uint32_t t0,
                                                  uint32_t (&best)[kMultiQB], uint32_t (&at)[kMultiQB], ReadB read_b) {
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) { // wave-uniform (a guard, not a break: the loop unrolls and best[] / at[] stay in registers)
            i32x8 A[4];
            query_operand<4>(qtab[qi].w[row], A);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if ((unsigned)u >= m) break; // wave-uniform
                i32x8 B[4];
                read_b(u, B);
                const uint32_t key = round_min_key(mfma_chain(A, B, c0, kBestScale));
                const bool better = (key | 15u) < best[qi]; // d below the best d
                best[qi] = better ? key : best[qi];
                at[qi] = better ? t0 + (uint32_t)u : at[qi];
            }
        }
    }
}

__device__ __forceinline__ unsigned long long best_key(uint32_t d, unsigned long long j) { return ((unsigned long long)d << kBestPosBits) | j; }

// The lane's (key, round counter) -> d << 58 | window.  The wave's counter t stands for round wave U + (t / U) nwaves U + t % U; lane (n, h), register r holds
// window 32 n + 8 (r >> 2) + 4 h + (r & 3) of it (distances_in_order's map); the rounds start at window `skip`.
template <int U>
__device__ __forceinline__ void best_lane_keys(const uint32_t (&best)[kMultiQB], const uint32_t (&at)[kMultiQB], unsigned lane, unsigned long long wave,
                                               unsigned long long nwaves, unsigned skip, unsigned long long (&key)[kMultiQB]) {
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        const uint32_t x = best[qi] & 0x7FFFFFu, r = x & 15u;
        const unsigned long long round = wave * U + (unsigned long long)(at[qi] / U) * nwaves * U + at[qi] % U;
        const unsigned long long j = skip + (round << 10) + 32u * (lane & 31u) + 8u * (r >> 2) + 4u * (lane >> 5) + (r & 3u);
        key[qi] = best[qi] == kBestNone ? kBestNoKey : best_key(x >> kBestShift, j);
    }
}

// The windows [0, pre) and [first, nwin), one per thread of the grid's x extent, every query of the block: word_of(j) is window j's 2-bit word
template <class Q, class WordOf>
__device__ __forceinline__ void best_tail_windows(unsigned long long pre, unsigned long long first, unsigned long long nwin, unsigned k,
                                                  const Q *__restrict__ queries, unsigned nq, unsigned long long (&key)[kMultiQB],
                                                  WordOf word_of) {
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
                const unsigned long long c = best_key(kind.dist(w, queries[qi]), j);
                key[qi] = c < key[qi] ? c : key[qi];
            }
        }
    }
}

// The end: per query, the wave's minimum, the workgroup's through LDS, one atomicMin per (workgroup, query) that saw a window
__device__ __forceinline__ void best_reduce(unsigned long long (&key)[kMultiQB], unsigned nq, unsigned lane, unsigned long long *__restrict__ keys) {
    __shared__ unsigned long long part[kMultiBlock / 64][kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) {
        if ((unsigned)qi < nq) {
            unsigned long long v = key[qi];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(v, off);
                v = o < v ? o : v;
            }
            if (lane == 0) part[threadIdx.x >> 6][qi] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < nq) {
        unsigned long long v = kBestNoKey;
        for (unsigned w = 0; w < (blockDim.x >> 6); ++w) v = part[w][threadIdx.x] < v ? part[w][threadIdx.x] : v;
        if (v != kBestNoKey) atomicMin(keys + threadIdx.x, v);
    }
}

// keys[q] -> pos[q], dist[q] (dist at any byte offset)
__global__ void __launch_bounds__(256) best_finish_kernel(const unsigned long long *__restrict__ keys, unsigned n_queries, unsigned long long *__restrict__ pos,
                                                          uint8_t *__restrict__ dist) {
    const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    const unsigned long long key = keys[q];
    const bool none = key == kBestNoKey;
    pos[q] = none ? kBestNoKey : key & ((1ull << kBestPosBits) - 1);
    dist[q] = none ? (uint8_t)0xFF : (uint8_t)(key >> kBestPosBits);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ASCII bytes at any alignment: the rounds start at ref + skip (16-byte aligned).
template <int U, class Q>
__global__ void __launch_bounds__(kMultiBlock)
kmer_best_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries,
                 unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys, unsigned long long *__restrict__ slot) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][AsciiStrip4<U>::kBytes];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    const bool latch = blockIdx.y == 0; // one query block reports invalid bytes
    best_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = ref + skip;
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const AsciiStrip4<U> fe(strips[wave_in_block()], lane);
    uint32_t best[kMultiQB], at[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) best[qi] = kBestNone, at[qi] = 0;

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
    const f32x16 c0 = best_acc_start();

    uint32_t t0 = 0; // the wave's round counter: + U per trip
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
        best_trip_queries<U>(qtab, nq, fe.row, m, c0, t0, best, at, [&](int u, i32x8 (&B)[4]) { fe.read_b(u, B); });
        r0 = rn;
        t0 += U;
    }

    unsigned long long key[kMultiQB];
    best_lane_keys<U>(best, at, lane, wave, nwaves, skip, key);
    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    best_tail_windows(pre, first, nwin, k, queries + q0, nq, key, [&](unsigned long long j) { return ascii_window_word(ref, j, k, latch, slot); });
    best_reduce(key, nq, lane, keys + q0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed words (8-byte aligned; at 8 mod 16 the rounds start one word later).
template <class Q>
__global__ void __launch_bounds__(kMultiBlock)
packed_best_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, const Q *__restrict__ queries,
                   unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][PackedStrip4::kBytes];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
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
    uint32_t best[kMultiQB], at[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) best[qi] = kBestNone, at[qi] = 0;

    unsigned long long r0 = wave * 4;
    PackedTrip cur;
    if (r0 < rounds) packed_trip_load(base, r0, rounds, lane, cur);
    const f32x16 c0 = best_acc_start();

    uint32_t t0 = 0;
    while (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, 4u);
        const unsigned long long rn = r0 + nwaves * 4;
        wave_lds_fence(); // the previous trip's readers are done
        fe.fill(lane, m, cur);
        if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
        wave_lds_fence();
        best_trip_queries<4>(qtab, nq, fe.row, m, c0, t0, best, at, [&](int u, i32x8 (&B)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) B[j] = PackedStrip4::operand(strip, rd[j], u);
        });
        r0 = rn;
        t0 += 4;
    }

    unsigned long long key[kMultiQB];
    best_lane_keys<4>(best, at, lane, wave, nwaves, skip, key);
    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    best_tail_windows(pre, first, nwin, k, queries + q0, nq, key, [&](unsigned long long j) { return packed_window_word(words, j, k); });
    best_reduce(key, nq, lane, keys + q0);
}

} // namespace bitnuc_dev
