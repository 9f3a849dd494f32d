// scan_packed_device.h -- the sliding k-mer Hamming scan and its fused count on PACKED 2-bit input (base i at bits 2 (i mod 32) of word i / 32):
// dist[j] = hdist_scalar(as_2bit(decode(w, n)[j .. j+k]), query, k), and the number of windows with dist <= tau.
//
// The contraction is scan_mfma_device.h's: a column is a segment of 32 consecutive windows, a row one of its 32 shifts, fp4 one-hot
// operands through v_mfma_scale_f32_32x32x64_f8f6f4, the accumulator biases and row scales pack the results.  The scan has four channels per base (four
// MFMAs per 1024 windows) and stores distance bytes as kmer_scan_seg_mfma_kernel does; the count has three (A, C, G one-hot, T = 0: three MFMAs per 1024
// windows), the d <= tau test inside the product and a bounded grid with the ticketed reduction, as kmer_count3_mfma_kernel.
//
// What differs is the front end: packed_trip_load, PackedStrip4 (scan, hit lists) and PackedStrip3 (count, multi-query count) below.  A round is still
// 1024 windows = 1024 bases, now 256 bytes; a lane's 16-byte load holds 64 bases, so one wave load of 1 KiB is exactly a trip of four rounds: lane l holds
// groups 4 (l & 15) + i (i = 0..3, 16 bases each, dword i of its load) of round l >> 4.  A code is already 2 bits: s_t = (x >> 2 t) & 0x03030303 puts bases
// t, t + 4, t + 8, t + 12 of a dword into byte lanes and one v_perm LUT per channel pair makes the nibbles; no byte can be invalid, so there is no
// validation and no error latch.  The (position, channel) order inside K that this produces is what the host tables follow (scan_packed_table /
// count3_packed_table, scan_mfma_host.h).
//
// The wave-private LDS strip is cut by group residue: the entry of group g of round u is entry 16 u + (g >> 2) of region g & 3 (per half for the scan, for
// the (A, C) bytes of the count), so lane l writes entry l of each of its regions -- one region per ds_write_b128, 64 consecutive 16-byte entries:
// conflict-free.  A K-step's readers take groups 2 n + c: two regions (residues r and r + 2) with four consecutive entries each per eight lanes; the two
// regions start 64 B mod 128 apart (region sizes of 32 mod 64 B), so those reads are conflict-free as well.  The count's G nibbles live in two regions by
// group PAIR parity with the same argument.  The halo (groups 0 and 1 of the round after the last valid one, the 32 bases after the trip) is two dwords,
// loaded by lanes 0 and 1 and written after the main entries (in-order LDS: the later write wins over a clamped copy).
//
// Alignment: the rounds read the words with 16-byte loads.  A words pointer at 8 mod 16 starts the rounds one word later; the first 32 windows then go to
// the tail threads (`skip` = 32), so the kernels need 8-byte aligned words only.  Distance bytes are stored with unaligned-capable 16-byte stores: any
// byte offset (gfx950 unaligned-access mode).  The windows that whole rounds do not cover, and all windows of n < 1056 (+ skip), are the tail threads'.
#pragma once
#include "device_prims.h"
#include "scan_mfma_device.h" // i32x8, f32x16, strip_operand, trip_rounds and the back end: query_operand ... hit_bits
#include "scan_mfma_host.h"

namespace bitnuc_dev {

constexpr int kPackedBlockScan = 64;   // packed_scan_mfma_kernel: one wave per workgroup (as the ASCII scan)
constexpr int kPackedRegion = 65 * 16 + 16;      // one residue region: 64 entries of a trip + the halo's, 32 mod 64 B (see the top of the file)
constexpr int kPackedGRegion = 65 * 16 + 48;     // one G-pair region of the count: 64 mod 128 B apart
static_assert((2 * kPackedRegion) % 128 == 64 && kPackedGRegion % 128 == 64, "regions read by one instruction must start 16 banks apart");

__device__ __forceinline__ uint32_t codes_at(uint32_t x, int t) { return (x >> (2 * t)) & 0x03030303u; } // bases t, t+4, t+8, t+12 in byte lanes
__device__ __forceinline__ uint32_t lut_ac(uint32_t s) { return __builtin_amdgcn_perm(0u, 0x00002002u, s); } // A (0) -> 0x02, C (1) -> 0x20
__device__ __forceinline__ uint32_t lut_gt(uint32_t s) { return __builtin_amdgcn_perm(0u, 0x20020000u, s); } // G (2) -> 0x02, T (3) -> 0x20

// window j as a 2-bit word: a funnel shift of two words; the second is read only where the window runs into it (sh > 0 then, and j + k - 1 < n keeps
// it in bounds)
__device__ __forceinline__ unsigned long long packed_window_word(const uint64_t *__restrict__ words, unsigned long long j, unsigned k) {
    const unsigned sh = 2u * (unsigned)(j & 31);
    unsigned long long x = words[j >> 5] >> sh;
    if ((j & 31) + k > 32) x |= words[(j >> 5) + 1] << (64 - sh);
    return x;
}

// the windows [0, pre) and [first, nwin): one window per thread, popcount of the differing fields (hamming/scalar.rs:33-47)
template <bool COUNT>
__device__ __forceinline__ uint32_t packed_tail_windows(const uint64_t *__restrict__ words, unsigned long long pre, unsigned long long first, unsigned long long nwin,
                                                        unsigned k, unsigned long long query, unsigned tau, uint8_t *__restrict__ dist) {
    const unsigned long long kmask = kmer_mask(k);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (nwin > first ? nwin - first : 0);
    uint32_t hits = 0;
    for (unsigned long long t = gt; t < total; t += nthreads) {
        const unsigned long long j = t < pre ? t : first + (t - pre);
        const uint32_t d = word_distance(packed_window_word(words, j, k), query, kmask);
        if constexpr (COUNT) hits += d <= tau ? 1u : 0u;
        else dist[j] = (uint8_t)d;
    }
    return hits;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The front end.  A trip in registers: the lane's 64 bases (groups 4 (l & 15) + i of round l >> 4) and, in lanes 0 and 1, the halo's dword (groups 0 and 1
// of the round after the last valid one).  `base` is 16-byte aligned; a round past the last valid one is a clamped copy of that one (redundant but in
// bounds).  hx keeps its value in lanes 2 .. 63: nothing reads it there.
struct PackedTrip {
    u32x4 x = u32x4{0u, 0u, 0u, 0u};
    uint32_t hx = 0;
};

__device__ __forceinline__ void packed_trip_load(const uint8_t *__restrict__ base, unsigned long long r0, unsigned long long rounds, unsigned lane, PackedTrip &t) {
    const unsigned m = trip_rounds(r0, rounds, 4u);
    const unsigned ul = lane >> 4, uc = ul < m ? ul : m - 1;
    t.x = load_group<true, true>(base + ((r0 + uc) << 8) + 16u * (lane & 15u));
    if (lane < 2) t.hx = *reinterpret_cast<const uint32_t *>(base + ((r0 + m) << 8) + 4u * lane);
}

// 16 bases (one packed dword) -> the four-channel operands of its two halves: half h = bases with (b & 3) >> 1 == h, (A, C) and (G, T) bytes of s_{2h}, s_{2h+1}
__device__ __forceinline__ void expand4_packed(uint32_t x, u32x4 &h0, u32x4 &h1) {
    const uint32_t s0 = codes_at(x, 0), s1 = codes_at(x, 1), s2 = codes_at(x, 2), s3 = codes_at(x, 3);
    h0 = u32x4{lut_ac(s0), lut_gt(s0), lut_ac(s1), lut_gt(s1)};
    h1 = u32x4{lut_ac(s2), lut_gt(s2), lut_ac(s3), lut_gt(s3)};
}

// Four channels per base.  Regions (half h, residue i) at (4 h + i) kPackedRegion.  Lane (n, h) of K-step j reads group G = 2 n + j: region
// 4 h + (G & 3), entry 16 u + (G >> 2).
struct PackedStrip4 {
    static constexpr int kBytes = 8 * kPackedRegion; // per wave
    uint8_t *strip;
    unsigned m32, hh; // lane (n, h) reads column n's operand of K-block h
    unsigned row;     // the lane's row of PackedScanTable: m - 2 h + 2
    __device__ __forceinline__ PackedStrip4(uint8_t *strip, unsigned lane) : strip(strip), m32(lane & 31u), hh(lane >> 5), row(m32 + 2u - 2u * hh) {}
    // rd[j]: where the lane reads K-step j of round 0.  The kernels keep the four in an array of their own, walk the K-steps themselves and hand operand()
    // their own strip: offsets held in this object, or read through its pointer, reach the optimiser as single-use sums, which it splits into chained
    // address adds; the kernels then recompute them per round or lose a wait (generated code is the judge: scan_mfma_device.h).
    __device__ __forceinline__ void read_offsets(unsigned (&rd)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned g = 2u * m32 + (unsigned)j;
            rd[j] = (4u * hh + (g & 3u)) * kPackedRegion + 16u * (g >> 2);
        }
    }
    static __device__ __forceinline__ void put(uint8_t *p, uint32_t x) {
        u32x4 e0, e1;
        expand4_packed(x, e0, e1);
        *reinterpret_cast<u32x4 *>(p) = e0;
        *reinterpret_cast<u32x4 *>(p + 4 * kPackedRegion) = e1;
    }
    // the lane's four groups (entry l of regions 0 .. 3 of each half), then the halo
    __device__ __forceinline__ void fill(unsigned lane, unsigned m, const PackedTrip &t) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) put(strip + i * kPackedRegion + 16u * lane, t.x[i]);
        if (lane < 2) put(strip + lane * kPackedRegion + 256u * m, t.hx);
    }
    // round u's operand of the K-step at offset rd
    static __device__ __forceinline__ i32x8 operand(const uint8_t *strip, unsigned rd, int u) { return strip_operand(strip + rd + 256u * u); }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// The distance bytes: one trip of four rounds per wave (the dispatcher walks the trips), workgroups of one wave.  Result order, pack and store: the back
// end's (pack_distances, store_distances), as the ASCII scan.
__global__ void __launch_bounds__(kPackedBlockScan) __attribute__((amdgpu_waves_per_eu(4, 8)))
packed_scan_mfma_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, unsigned long long query, uint8_t *__restrict__ dist,
                        const PackedScanTable tab) {
    __shared__ __attribute__((aligned(16))) uint8_t strip[PackedStrip4::kBytes];
    const unsigned long long nwin = n - k + 1;
    const unsigned long long pre = skip < nwin ? skip : nwin; // windows before the rounds: the tail threads'
    const unsigned long long rounds = scan_rounds(n, skip);    // skip = 0 or 32
    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5)); // 16-byte aligned
    uint8_t *dst = dist + skip;
    const unsigned lane = threadIdx.x & 63;
    const PackedStrip4 fe(strip, lane);
    const unsigned long long r0 = (unsigned long long)blockIdx.x * 4;
    if (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, 4u);
        PackedTrip cur;
        packed_trip_load(base, r0, rounds, lane, cur);
        i32x8 A[4];
        query_operand<4>(tab.w[fe.row], A);
        const int scale_a = dist_row_scale(fe.m32);
        const f32x16 c0 = acc_start(tab.c); // 2^23
        fe.fill(lane, m, cur);
        unsigned rd[4]; // (here and not in fe: read_offsets' note)
        fe.read_offsets(rd);
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((unsigned)u >= m) break; // wave-uniform
            i32x8 B[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) B[j] = PackedStrip4::operand(strip, rd[j], u);
            uint32_t o[4];
            pack_distances(mfma_chain(A, B, c0, scale_a), o);
            store_distances<true, false>(dst + ((r0 + u) << 10) + 16u * (2u * fe.m32 + fe.hh), o);
        }
    }
    packed_tail_windows<false>(words, pre, skip + (rounds << 10), nwin, k, query, 0u, dist);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Three channels per base (the fused count).  The (A, C) bytes in regions by residue (lane l writes entry l of region i: lut_ac(s_0..s_3) of its dword i),
// the G nibbles in two regions by pair parity (lane l writes entry l of region 0 with groups 4 (l & 15), + 1 and of region 1 with + 2, + 3; a group's G
// nibbles are two dwords: nibble p of the even / odd one = base 2 p / 2 p + 1).  K-step s < 2 of lane (n, h) reads the (A, C) bytes of group
// G = 2 n + 2 s + h (region G & 3, entry 16 u + (G >> 2)); K-step 2 the G nibbles of groups 2 (n + h), + 1 (region (n + h) & 1, entry
// 16 u + ((n + h) >> 1)).
__device__ __forceinline__ void g_nibbles(uint32_t x, uint32_t &ge, uint32_t &go) {
    const uint32_t y = x & ~(x << 1) & 0xAAAAAAAAu; // bit 2 b + 1 set <=> base b is G (code 2)
    ge = y & 0x22222222u;                           // nibble p = base 2 p
    go = (y >> 2) & 0x22222222u;                    // nibble p = base 2 p + 1
}

struct PackedStrip3 {
    static constexpr int kG0 = 4 * kPackedRegion;                  // where the G regions start
    static constexpr int kBytes = kG0 + 2 * kPackedGRegion;        // per wave
    uint8_t *strip;
    unsigned rd[3]; // K-step s of round u: + 256 u
    __device__ __forceinline__ PackedStrip3(uint8_t *strip, unsigned lane) : strip(strip) {
        const unsigned m32 = lane & 31u, hh = lane >> 5;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned g = 2u * m32 + 2u * (unsigned)s + hh;
            rd[s] = (g & 3u) * kPackedRegion + 16u * (g >> 2);
        }
        rd[2] = kG0 + ((m32 + hh) & 1u) * kPackedGRegion + 16u * ((m32 + hh) >> 1);
    }
    static __device__ __forceinline__ u32x4 ac_bytes(uint32_t x) { return u32x4{lut_ac(codes_at(x, 0)), lut_ac(codes_at(x, 1)), lut_ac(codes_at(x, 2)), lut_ac(codes_at(x, 3))}; }
    // the lane's four groups, then the halo
    __device__ __forceinline__ void fill(unsigned lane, unsigned m, const PackedTrip &t) const {
        uint32_t ge[4], go[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<u32x4 *>(strip + i * kPackedRegion + 16u * lane) = ac_bytes(t.x[i]);
            g_nibbles(t.x[i], ge[i], go[i]);
        }
        *reinterpret_cast<u32x4 *>(strip + kG0 + 16u * lane) = u32x4{ge[0], go[0], ge[1], go[1]};
        *reinterpret_cast<u32x4 *>(strip + kG0 + kPackedGRegion + 16u * lane) = u32x4{ge[2], go[2], ge[3], go[3]};
        if (lane < 2) {
            *reinterpret_cast<u32x4 *>(strip + lane * kPackedRegion + 256u * m) = ac_bytes(t.hx);
            uint32_t he, ho;
            g_nibbles(t.hx, he, ho);
            *reinterpret_cast<u32x2 *>(strip + kG0 + 256u * m + 8u * lane) = u32x2{he, ho};
        }
    }
    __device__ __forceinline__ void read_b(int u, i32x8 (&B)[3]) const {
#pragma unroll
        for (int j = 0; j < 3; ++j) B[j] = strip_operand(strip + rd[j] + 256u * u);
    }
};

// Threshold fields and hit bits: the back end's.  The next trip is loaded into the same registers during the matrix phase and the workgroups' sums meet at
// a ticket, as in the ASCII count.
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 8)))
packed_count3_mfma_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, unsigned long long query, unsigned tau,
                          unsigned long long *__restrict__ result, unsigned long long *__restrict__ total /* zero between launches */,
                          unsigned *__restrict__ ticket, const Count3MfmaTable tab) {
    __shared__ __attribute__((aligned(16))) uint8_t strips[kBlock / 64][PackedStrip3::kBytes];
    const unsigned long long nwin = n - k + 1;
    const unsigned long long pre = skip < nwin ? skip : nwin; // windows before the rounds: the tail threads'
    const unsigned long long rounds = scan_rounds(n, skip);    // skip = 0 or 32
    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const PackedStrip3 fe(strips[wave_in_block()], lane);

    unsigned long long r0 = wave * 4;
    PackedTrip cur;
    if (r0 < rounds) packed_trip_load(base, r0, rounds, lane, cur);
    i32x8 A[3];
    query_operand<3>(tab.w[lane], A);
    asm volatile("" : "+v"(A[0][0]), "+v"(A[0][1]), "+v"(A[0][2]), "+v"(A[0][3]), "+v"(A[1][0]), "+v"(A[1][1]), "+v"(A[1][2]), "+v"(A[1][3]),
                      "+v"(A[2][0]), "+v"(A[2][1]), "+v"(A[2][2]), "+v"(A[2][3]));
    uint32_t lane_hits = 0;
    const int scale_a = count_row_scale(lane & 31u);
    const f32x16 c0 = acc_start(tab.c);

    while (r0 < rounds) {
        const unsigned m = trip_rounds(r0, rounds, 4u);
        const unsigned long long rn = r0 + nwaves * 4;
        wave_lds_fence(); // the previous trip's readers are done
        fe.fill(lane, m, cur);
        if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((unsigned)u >= m) break; // wave-uniform
            i32x8 B[3];
            fe.read_b(u, B);
            const f32x16 acc = mfma_chain(A, B, c0, scale_a);
#pragma unroll
            for (int q = 0; q < 4; ++q) lane_hits += (uint32_t)__builtin_popcount(hit_bits(acc, q));
        }
        r0 = rn;
    }

    uint32_t hits = packed_tail_windows<true>(words, pre, skip + (rounds << 10), nwin, k, query, tau, nullptr) + lane_hits;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off);
    __shared__ uint32_t part[kBlock / 64];
    if (lane == 0) part[threadIdx.x >> 6] = hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (unsigned i = 0; i < (blockDim.x >> 6); ++i) s += part[i];
        if (s) add_performed(total, s);
        if (draw_last_ticket(ticket)) *result = atomicExch(total, 0ull);
    }
}

} // namespace bitnuc_dev
