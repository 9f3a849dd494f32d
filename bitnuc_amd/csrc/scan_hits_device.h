// scan_hits_device.h -- the positions of the k-mer windows within a Hamming threshold: pos[0 .. min(cap, total)) = the windows j with
// hdist_scalar(as_2bit(ref[j .. j+k]), query, k) <= tau in ascending order, hit_dist[r] = the distance of window pos[r], *n_hits = total.
//
// Three stream-ordered launches, no workgroup ever waits for another:
//   1. kmer_hits_mfma_kernel<false> / packed_hits_mfma_kernel<false>: the count pass.  One workgroup of one wave per TRIP (the scan's unit: four rounds
//      of 1024 windows + the 32-byte halo) runs the scan's contraction (scan_mfma_device.h: the segment tiling, four channels per base, pack_distances),
//      compares the four distance bytes of a dword with tau in two instructions (hits_of4) and writes the trip's number of hits to counts[1 + trip].
//      The first workgroup takes the head windows before the first 16-byte aligned base, the last one the windows after the last whole round, one
//      window per lane: counts[] is in window order.
//   2. hits_scan_tiles_kernel + hits_scan_top_kernel: the exclusive scan of the per-trip counts (244 K entries at 10^9 bases) in tiles of 4096, then
//      the tiles' totals in one workgroup, which also writes *n_hits.
//   3. the same kernels <true>: the emit pass.  Each trip is recomputed; a round's 1024 hit bits are put in window order (store_distances' two
//      v_permlane32_swap give lane (n, h) the windows 32 n + 16 h .. + 16, a ds_bpermute moves that chunk to lane 2 n + h), a wave prefix over the
//      lanes' popcounts ranks them, and pos / hit_dist are written at the trip's offset plus the rank, nothing at or beyond cap.  A round without a
//      hit costs one ballot.  The tail is ranked with v_mbcnt over a ballot per 64 windows.
// The passes compute the same distances from the same bytes with the same instructions: the emit pass writes exactly the hits the count pass counted.
#pragma once
#include "device_prims.h"
#include "scan_mfma_device.h"   // the back end: query_operand, acc_start, mfma_chain, pack_distances, distances_in_order; the front end: AsciiStrip4
#include "scan_packed_device.h" // the packed front end: PackedStrip4
#include "scan_mfma_host.h"

namespace bitnuc_dev {

constexpr int kHitsRounds = 4;           // rounds per trip = per workgroup of one wave
constexpr unsigned kHitsTile = 4096;     // per-trip counts per workgroup of the tile scan (256 threads x 16)
constexpr int kHitsTileBlock = 256;
constexpr int kHitsTopBlock = 1024;

// trips of n bases whose first `skip` windows are taken apart; the count / emit grid is trips + 2, in window order: workgroup 0 takes the head
// windows [0, skip), workgroup 1 + t trip t, the last one the tail
constexpr unsigned long long hits_trips(unsigned long long n, unsigned skip) { return (scan_rounds(n, skip) + kHitsRounds - 1) / kHitsRounds; }

// bit 7 of byte i set <=> distance byte i of d is <= t, with bias = 0x7F7F7F7F - t 0x01010101 and t <= 32 (a byte stays in 95 .. 159: no carry)
__device__ __forceinline__ uint32_t hits_of4(uint32_t d, uint32_t bias) { return ~(d + bias) & 0x80808080u; }
__device__ __forceinline__ uint32_t hits_bias(unsigned tau) { return 0x7F7F7F7Fu - (tau < 32u ? tau : 32u) * 0x01010101u; }
// bits 7, 15, 23, 31 -> bits 0 .. 3
__device__ __forceinline__ uint32_t hit_nibble(uint32_t h) {
    uint32_t x = h >> 7;
    x |= x >> 7;
    x |= x >> 14;
    return x & 0xFu;
}

// the count pass's hits of one round (any lane order)
__device__ __forceinline__ uint32_t round_hits(const f32x16 &acc, uint32_t bias) {
    uint32_t o[4];
    pack_distances(acc, o);
    uint32_t h = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) h += (uint32_t)__builtin_popcount(hits_of4(o[q], bias));
    return h;
}

// The emit pass's round: write the hits of windows first + 0 .. 1023 at ranks rank, rank + 1, ... (rank: wave-uniform, advanced by the round's hits)
__device__ __forceinline__ void emit_round(const f32x16 &acc, uint32_t bias, unsigned lane, unsigned long long first, unsigned long long &rank,
                                           unsigned long long cap, unsigned long long *__restrict__ pos, uint8_t *__restrict__ hd) {
    u32x4 v = distances_in_order(acc); // lane (n, h): windows 32 n + 16 h .. + 16
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m |= hit_nibble(hits_of4(v[i], bias)) << (4 * i);
    if (__ballot(m != 0u) == 0ull) return; // wave-uniform
    // window order: lane c takes chunk c = 2 n + h from lane n + 32 h
    const int src = (int)((lane >> 1) + 32u * (lane & 1u));
    m = (uint32_t)__shfl((int)m, src);
    if (hd) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (uint32_t)__shfl((int)v[i], src);
    }
    const uint32_t p = (uint32_t)__builtin_popcount(m);
    uint32_t s = p; // inclusive prefix over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)s, off);
        if (lane >= (unsigned)off) s += t;
    }
    const uint32_t round_total = (uint32_t)__shfl((int)s, 63);
    unsigned long long r = rank + (s - p);
    const unsigned long long w0 = first + 16ull * lane;
    while (m) {
        const unsigned i = (unsigned)__builtin_ctz(m);
        if (r < cap) {
            pos[r] = w0 + i;
            if (hd) {
                const uint32_t dw = i < 8 ? (i < 4 ? v[0] : v[1]) : (i < 12 ? v[2] : v[3]);
                hd[r] = (uint8_t)(dw >> (8 * (i & 3)));
            }
        }
        ++r;
        m &= m - 1;
    }
    rank += round_total;
}

// The windows [0, pre) and [first, nwin) of one wave, 64 at a time in window order: dist_of(j) is window j's distance.  Count pass: returns the lane's
// hits.  Emit pass: ranks them with v_mbcnt from `rank` and writes those below cap.
template <bool EMIT, class DistOf>
__device__ __forceinline__ uint32_t hits_tail(unsigned long long pre, unsigned long long first, unsigned long long nwin, unsigned tau, unsigned lane,
                                              unsigned long long rank, unsigned long long cap, unsigned long long pos_base,
                                              unsigned long long *__restrict__ pos, uint8_t *__restrict__ hd, DistOf dist_of) {
    const unsigned long long total = pre + (nwin > first ? nwin - first : 0);
    uint32_t hits = 0;
    for (unsigned long long t0 = 0; t0 < total; t0 += 64) {
        const unsigned long long t = t0 + lane;
        const unsigned long long j = t < pre ? t : first + (t - pre);
        uint32_t d = 0;
        bool hit = false;
        if (t < total) {
            d = dist_of(j);
            hit = d <= tau;
        }
        if constexpr (EMIT) {
            const unsigned long long b = __ballot(hit);
            const unsigned long long r = rank + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (hit && r < cap) {
                pos[r] = pos_base + j;
                if (hd) hd[r] = (uint8_t)d;
            }
            rank += (unsigned long long)__builtin_popcountll(b);
        } else {
            hits += hit ? 1u : 0u;
        }
    }
    return hits;
}

// the count pass's end: the wave's hits -> counts[blockIdx.x]
__device__ __forceinline__ void write_hit_count(uint32_t hits, unsigned lane, unsigned *__restrict__ counts) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off);
    if (lane == 0) counts[blockIdx.x] = hits;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ASCII input.  The rounds start at ref + skip, 16-byte aligned (skip = (-ref) mod 16; the first skip windows are the first workgroup's), so any ref runs these
// kernels.  Front end: AsciiStrip4 (U = 4), as the scan.  Invalid bytes are latched by the count pass only: trip_invalid over the
// trip's rounds, byte loads in the tail (scan_tail_windows' rule), so the slot holds the first invalid byte of the whole sequence, as the count's.
// EMIT: counts[] holds the exclusive offsets within a tile, tile_off[] the tiles' (hits_scan_*).
// Q: the query kind (QueryKind, scan_mfma_device.h); the table is the caller's (scan_seg_table of either kind)
template <bool EMIT, class Q>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8)))
kmer_hits_mfma_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned k, const Q query, unsigned tau,
                      unsigned *__restrict__ counts, const unsigned long long *__restrict__ tile_off, unsigned long long *__restrict__ pos,
                      uint8_t *__restrict__ hd, unsigned long long cap, unsigned long long pos_base, unsigned long long *__restrict__ slot,
                      const CountMfmaTable tab) {
    constexpr int U = kHitsRounds;
    __shared__ __attribute__((aligned(16))) uint8_t strip[AsciiStrip4<U>::kBytes];
    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const unsigned long long blk = blockIdx.x, trip = blk - 1;
    const unsigned lane = threadIdx.x & 63;
    const AsciiStrip4<U> fe(strip, lane);
    const uint32_t bias = hits_bias(tau);
    unsigned long long rank = 0;
    if constexpr (EMIT) rank = tile_off[blk / kHitsTile] + counts[blk];
    uint32_t hits = 0;
    if (blk != 0 && trip < (rounds + U - 1) / U) {
        const uint8_t *base = ref + skip;
        const unsigned long long r0 = trip * U;
        ScanTrip<U> cur;
        scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
        const unsigned m = trip_rounds(r0, rounds, U);
        i32x8 A[4];
        query_operand<4>(tab.w[fe.row], A);
        const int scale_a = dist_row_scale(lane & 31u);
        const f32x16 c0 = acc_start(tab.c); // 2^23
        const uint32_t trip_bad = fe.fill(lane, m, cur);
        if (!EMIT && __builtin_expect(trip_invalid(trip_bad), 0)) {
#pragma unroll 1
            for (unsigned u = 0; u < m; ++u) rescan_bytes(ref, skip + ((r0 + u) << 10) + 16 * lane, 16, slot);
        }
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if ((unsigned)u >= m) break; // wave-uniform
            i32x8 B[4];
            fe.read_b(u, B);
            const f32x16 acc = mfma_chain(A, B, c0, scale_a);
            if constexpr (EMIT) emit_round(acc, bias, lane, pos_base + skip + ((r0 + u) << 10), rank, cap, pos, hd);
            else hits += round_hits(acc, bias);
        }
    } else { // the first workgroup: the head windows [0, skip); the last: the tail
        const QueryKind<Q> kind(k);
        const unsigned long long pre = blk == 0 ? (skip < nwin ? skip : nwin) : 0, first = blk == 0 ? nwin : skip + (rounds << 10);
        hits = hits_tail<EMIT>(pre, first, nwin, tau, lane, rank, cap, pos_base, pos, hd,
                               [&](unsigned long long j) { return kind.dist(kind.window(ascii_window_word(ref, j, k, !EMIT, slot)), query); });
    }
    if constexpr (!EMIT) write_hit_count(hits, lane, counts);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed input: packed_trip_load and PackedStrip4, as the packed scan (one wave load of 1 KiB = one trip, strip cut by group residue); words at 8 mod 16
// start the rounds one word later (skip = 32).  No byte can be invalid.
template <bool EMIT, class Q>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8)))
packed_hits_mfma_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned k, const Q query, unsigned tau,
                        unsigned *__restrict__ counts, const unsigned long long *__restrict__ tile_off, unsigned long long *__restrict__ pos,
                        uint8_t *__restrict__ hd, unsigned long long cap, unsigned long long pos_base, const PackedScanTable tab) {
    __shared__ __attribute__((aligned(16))) uint8_t strip[PackedStrip4::kBytes];
    const unsigned long long nwin = n - k + 1;
    const unsigned long long rounds = scan_rounds(n, skip);
    const unsigned long long blk = blockIdx.x, trip = blk - 1;
    const unsigned lane = threadIdx.x & 63;
    const PackedStrip4 fe(strip, lane);
    const uint32_t bias = hits_bias(tau);
    unsigned long long rank = 0;
    if constexpr (EMIT) rank = tile_off[blk / kHitsTile] + counts[blk];
    uint32_t hits = 0;
    if (blk != 0 && trip < (rounds + 3) / 4) {
        const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5)); // 16-byte aligned
        const unsigned long long r0 = trip * 4;
        const unsigned m = trip_rounds(r0, rounds, 4u);
        PackedTrip cur;
        packed_trip_load(base, r0, rounds, lane, cur);
        i32x8 A[4];
        query_operand<4>(tab.w[fe.row], A);
        const int scale_a = dist_row_scale(lane & 31u);
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
            const f32x16 acc = mfma_chain(A, B, c0, scale_a);
            if constexpr (EMIT) emit_round(acc, bias, lane, pos_base + skip + ((r0 + u) << 10), rank, cap, pos, hd);
            else hits += round_hits(acc, bias);
        }
    } else { // the head windows [0, skip), the tail
        const QueryKind<Q> kind(k);
        const unsigned long long pre = blk == 0 ? (skip < nwin ? skip : nwin) : 0, first = blk == 0 ? nwin : skip + (rounds << 10);
        hits = hits_tail<EMIT>(pre, first, nwin, tau, lane, rank, cap, pos_base, pos, hd,
                               [&](unsigned long long j) { return kind.dist(kind.window(packed_window_word(words, j, k)), query); });
    }
    if constexpr (!EMIT) write_hit_count(hits, lane, counts);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The exclusive scan of the per-trip counts.  Tiles: thread t of tile b owns entries 4096 b + 16 t .. + 16, rewrites them as offsets within the tile
// (a tile holds at most 4096 x 4096 hits: u32) and the tile's total goes to tile_sum[b].  Top: one workgroup turns tile_sum into exclusive offsets
// (1024 at a time, carried) and writes the grand total to *n_hits.
__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long s, unsigned lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(s, off);
        if (lane >= (unsigned)off) s += t;
    }
    return s;
}

__global__ void __launch_bounds__(kHitsTileBlock) hits_scan_tiles_kernel(unsigned *__restrict__ counts, unsigned long long ntr, unsigned long long *__restrict__ tile_sum) {
    __shared__ unsigned long long wsum[kHitsTileBlock / 64];
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * kHitsTile + 16ull * threadIdx.x;
    uint32_t c[16];
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t v = e0 + i < ntr ? counts[e0 + i] : 0u;
        c[i] = s;
        s += v;
    }
    const unsigned long long incl = wave_inclusive_scan(s, lane);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned long long off = incl - s;
    for (unsigned w = 0; w < wv; ++w) off += wsum[w];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (e0 + i < ntr) counts[e0 + i] = (uint32_t)off + c[i];
    if (threadIdx.x == kHitsTileBlock - 1) tile_sum[blockIdx.x] = off + s;
}

__global__ void __launch_bounds__(kHitsTopBlock) hits_scan_top_kernel(unsigned long long *__restrict__ tile_sum, unsigned long long ntiles, unsigned long long *__restrict__ n_hits) {
    __shared__ unsigned long long wsum[kHitsTopBlock / 64];
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (unsigned long long b0 = 0; b0 < ntiles; b0 += kHitsTopBlock) {
        const unsigned long long i = b0 + threadIdx.x;
        const unsigned long long v = i < ntiles ? tile_sum[i] : 0ull;
        const unsigned long long incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        unsigned long long off = carry + incl - v, all = 0;
        for (unsigned w = 0; w < kHitsTopBlock / 64; ++w) {
            if (w < wv) off += wsum[w];
            all += wsum[w];
        }
        if (i < ntiles) tile_sum[i] = off;
        carry += all;
        __syncthreads(); // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *n_hits = carry;
}

} // namespace bitnuc_dev
