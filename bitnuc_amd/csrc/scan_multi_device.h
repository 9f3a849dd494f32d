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
//   * front end, strip layout, invalid-byte rule, next-trip prefetch: kmer_count3_mfma_kernel's (ASCII) and packed_count3_mfma_kernel's (packed);
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
#include "scan_mfma_device.h"   // ScanTrip, scan_trip_load, expand3 and the back end: query_operand, acc_start, count_row_scale, mfma_chain, hit_bits
#include "scan_packed_device.h" // the packed front end: codes_at, lut_ac, g_nibbles, kPackedRegion, kPackedGRegion
#include "scan_mfma_host.h"     // Count3Rule, count3_mfma_lane, count3_packed_lane

namespace bitnuc_dev {

constexpr int kMultiQB = 16;     // queries per workgroup (grid.y block): one per-lane counter each
constexpr int kMultiBlock = 768; // threads per workgroup: 12 waves, one workgroup per CU (its LDS: 16 tables + 12 strips)
constexpr int kMultiRounds = 4;  // rounds per trip (ASCII; a packed trip is one 1 KiB wave load = 4 rounds)
static_assert(sizeof(Count3MfmaTable) % 16 == 0, "tables are copied and read as 16-byte pieces");
using bitnuc_host::Count3Rule;

// One thread per (query, lane): lane's 12 dwords of query q's table, lane 0 also its start values
template <bool PACKED>
__global__ void __launch_bounds__(64) count3_tables_kernel(const unsigned long long *__restrict__ queries, const unsigned *__restrict__ taus, unsigned k,
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

// Every query of the block against one round's B operand: hits[qi] += the round's windows with d <= tau_qi (lane's share).  The query loop is outside
// the round loop at the call site: a query's A operand and start values are read once per trip.
template <int U, class ReadB>
__device__ __forceinline__ void multi_trip_queries(const Count3MfmaTable *qtab, unsigned nq, unsigned lane, unsigned m, int scale_a, uint32_t (&hits)[kMultiQB],
                                                   ReadB read_b) {
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
                read_b(u, B);
                const f32x16 acc = mfma_chain(A, B, c0, scale_a);
#pragma unroll
                for (int q = 0; q < 4; ++q) hits[qi] += (uint32_t)__builtin_popcount(hit_bits(acc, q));
            }
        }
    }
}

// The windows [0, pre) and [first, nwin), one per thread of the grid's x extent, every query of the block: word_of(j) is window j's 2-bit word
template <class WordOf>
__device__ __forceinline__ void multi_tail_windows(unsigned long long pre, unsigned long long first, unsigned long long nwin, unsigned k,
                                                   const unsigned long long *__restrict__ queries, const unsigned *__restrict__ taus, unsigned nq,
                                                   uint32_t (&hits)[kMultiQB], WordOf word_of) {
    const unsigned long long kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (nwin > first ? nwin - first : 0);
    for (unsigned long long t = gt; t < total; t += nthreads) {
        const unsigned long long j = t < pre ? t : first + (t - pre);
        const unsigned long long w = word_of(j);
#pragma unroll
        for (int qi = 0; qi < kMultiQB; ++qi) {
            if ((unsigned)qi < nq) {
                const unsigned long long x = (w ^ queries[qi]) & kmask;
                const uint32_t d = (uint32_t)__builtin_popcountll((x | (x >> 1)) & 0x5555555555555555ull);
                hits[qi] += d <= taus[qi] ? 1u : 0u;
            }
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
// ASCII bytes at any alignment: the rounds start at ref + skip (16-byte aligned).  Strip and offsets: kmer_count3_mfma_kernel's.
template <int U>
__global__ void __launch_bounds__(kMultiBlock)
kmer_count3_multi_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned k, const unsigned long long *__restrict__ queries,
                         const unsigned *__restrict__ taus, unsigned n_queries, const Count3MfmaTable *__restrict__ tabs,
                         unsigned long long *__restrict__ counts, unsigned long long *__restrict__ slot) {
    constexpr int kAc = (32 * U + 1) * 16 + 48; // (kmer_count3_mfma_kernel's regions)
    static_assert(kAc % 128 == 64, "the two parities of one store must land 16 banks apart");
    constexpr int kG = (32 * U + 1) * 16;
    __shared__ __attribute__((aligned(16))) Count3MfmaTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][2 * kAc + kG];
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
    uint8_t *strip = strips[wave_in_block()];
    uint32_t hits[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) hits[qi] = 0;

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
    const unsigned m32 = lane & 31u, hh = lane >> 5;
    const int scale_a = count_row_scale(m32);
    const unsigned wr_ac = (lane & 1u) * kAc + 16u * (lane >> 1);
    const unsigned wr_g = 2u * kAc + 8u * lane;
    const unsigned rd_ac = hh * kAc + 16u * m32;
    const unsigned rd_g = 2u * kAc + 16u * (m32 + hh);

    while (r0 < rounds) {
        const unsigned m = rounds - r0 < (unsigned long long)U ? (unsigned)(rounds - r0) : (unsigned)U;
        const unsigned long long rn = r0 + nwaves * U;
        wave_lds_fence(); // the previous trip's readers are done
        uint32_t trip_bad = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = cur.v[u][0];
#pragma unroll
            for (int i = 0; i < 4; ++i) trip_bad |= x[i] ^ __builtin_amdgcn_perm(0x47FFFF54u, 0x43FF41FFu, x[i] & 0x07070707u); // (trip_invalid's LUT)
            u32x4 ac;
            uint32_t g0, g1;
            expand3(x, ac, g0, g1);
            *reinterpret_cast<u32x4 *>(strip + wr_ac + 512 * u) = ac;
            *reinterpret_cast<u32x2 *>(strip + wr_g + 512 * u) = u32x2{g0, g1};
        }
        if (lane < 2) { // the halo (kmer_count3_mfma_kernel's)
            u32x4 ac;
            uint32_t g0, g1;
            expand3(cur.hv, ac, g0, g1);
            *reinterpret_cast<u32x4 *>(strip + lane * kAc + 512 * m) = ac;
            *reinterpret_cast<u32x2 *>(strip + 2 * kAc + 512 * m + 8 * lane) = u32x2{g0, g1};
        }
        if (latch && __builtin_expect(trip_invalid(trip_bad), 0)) {
#pragma unroll 1
            for (unsigned u = 0; u < m; ++u) rescan_bytes(ref, skip + ((r0 + u) << 10) + 16 * lane, 16, slot);
        }
        if (rn < rounds) scan_trip_load<U, 3, true>(base, rn, rounds, lane, cur); // cur's bytes are in the strip: its registers take the next trip
        wave_lds_fence();
        multi_trip_queries<U>(qtab, nq, lane, m, scale_a, hits, [&](int u, i32x8 (&B)[3]) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x4 t = *reinterpret_cast<const u32x4 *>(strip + (j < 2 ? rd_ac + 16 * j : rd_g) + 512 * u);
                B[j] = i32x8{(int)t.x, (int)t.y, (int)t.z, (int)t.w, 0, 0, 0, 0};
            }
        });
        r0 = rn;
    }

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    multi_tail_windows(pre, first, nwin, k, queries + q0, taus + q0, nq, hits, [&](unsigned long long j) {
        unsigned long long w = 0;
        bool flagged = false;
        for (unsigned b = 0; b < k; ++b) {
            const uint32_t byte = ref[j + b];
            if (latch && !valid_base(byte) && !flagged) { latch_bad(slot, j + b, byte); flagged = true; }
            w |= (unsigned long long)code_of(byte) << (2 * b);
        }
        return w;
    });
    multi_reduce(hits, nq, lane, counts + q0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed words (8-byte aligned; at 8 mod 16 the rounds start one word later).  Front end and strip: packed_count3_mfma_kernel's.
__global__ void __launch_bounds__(kMultiBlock)
packed_count3_multi_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, const unsigned long long *__restrict__ queries,
                           const unsigned *__restrict__ taus, unsigned n_queries, const Count3MfmaTable *__restrict__ tabs,
                           unsigned long long *__restrict__ counts) {
    constexpr int kG0 = 4 * kPackedRegion;
    __shared__ __attribute__((aligned(16))) Count3MfmaTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][4 * kPackedRegion + 2 * kPackedGRegion];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    multi_tables_to_lds(tabs + q0, nq, qtab);

    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    uint8_t *strip = strips[wave_in_block()];
    const unsigned ul = lane >> 4;
    uint32_t hits[kMultiQB];
#pragma unroll
    for (int qi = 0; qi < kMultiQB; ++qi) hits[qi] = 0;

    unsigned long long r0 = wave * 4;
    u32x4 x = u32x4{0u, 0u, 0u, 0u};
    uint32_t hx = 0;
    auto load_trip = [&](unsigned long long r) {
        const unsigned m = rounds - r < 4ull ? (unsigned)(rounds - r) : 4u;
        const unsigned uc = ul < m ? ul : m - 1;
        x = load_group<true, true>(base + ((r + uc) << 8) + 16u * (lane & 15u));
        if (lane < 2) hx = *reinterpret_cast<const uint32_t *>(base + ((r + m) << 8) + 4u * lane);
    };
    if (r0 < rounds) load_trip(r0);
    const unsigned m32 = lane & 31u, hh = lane >> 5;
    const int scale_a = count_row_scale(m32);
    unsigned rd[3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned g = 2u * m32 + 2u * (unsigned)s + hh;
        rd[s] = (g & 3u) * kPackedRegion + 16u * (g >> 2);
    }
    rd[2] = kG0 + ((m32 + hh) & 1u) * kPackedGRegion + 16u * ((m32 + hh) >> 1);

    while (r0 < rounds) {
        const unsigned m = rounds - r0 < 4ull ? (unsigned)(rounds - r0) : 4u;
        const unsigned long long rn = r0 + nwaves * 4;
        wave_lds_fence(); // the previous trip's readers are done
        uint32_t ge[4], go[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t xi = x[i];
            *reinterpret_cast<u32x4 *>(strip + i * kPackedRegion + 16u * lane) =
                u32x4{lut_ac(codes_at(xi, 0)), lut_ac(codes_at(xi, 1)), lut_ac(codes_at(xi, 2)), lut_ac(codes_at(xi, 3))};
            g_nibbles(xi, ge[i], go[i]);
        }
        *reinterpret_cast<u32x4 *>(strip + kG0 + 16u * lane) = u32x4{ge[0], go[0], ge[1], go[1]};
        *reinterpret_cast<u32x4 *>(strip + kG0 + kPackedGRegion + 16u * lane) = u32x4{ge[2], go[2], ge[3], go[3]};
        if (lane < 2) { // the halo: groups 0 and 1 of round m
            *reinterpret_cast<u32x4 *>(strip + lane * kPackedRegion + 256u * m) =
                u32x4{lut_ac(codes_at(hx, 0)), lut_ac(codes_at(hx, 1)), lut_ac(codes_at(hx, 2)), lut_ac(codes_at(hx, 3))};
            uint32_t he, ho;
            g_nibbles(hx, he, ho);
            *reinterpret_cast<u32x2 *>(strip + kG0 + 256u * m + 8u * lane) = u32x2{he, ho};
        }
        if (rn < rounds) load_trip(rn); // x's bases are in the strip: its registers take the next trip
        wave_lds_fence();
        multi_trip_queries<4>(qtab, nq, lane, m, scale_a, hits, [&](int u, i32x8 (&B)[3]) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x4 t = *reinterpret_cast<const u32x4 *>(strip + rd[j] + 256u * u);
                B[j] = i32x8{(int)t.x, (int)t.y, (int)t.z, (int)t.w, 0, 0, 0, 0};
            }
        });
        r0 = rn;
    }

    const unsigned long long pre = skip < nwin ? skip : nwin, first = skip + (rounds << 10);
    multi_tail_windows(pre, first, nwin, k, queries + q0, taus + q0, nq, hits, [&](unsigned long long j) {
        const unsigned sh = 2u * (unsigned)(j & 31);
        unsigned long long w = words[j >> 5] >> sh;
        if ((j & 31) + k > 32) w |= words[(j >> 5) + 1] << (64 - sh); // (packed_tail_windows' funnel: in bounds since j + k - 1 < n)
        return w;
    });
    multi_reduce(hits, nq, lane, counts + q0);
}

} // namespace bitnuc_dev
