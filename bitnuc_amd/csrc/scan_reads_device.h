// scan_reads_device.h -- the best match per READ of a fixed-length batch: for every read r the lexicographically smallest (distance, query, offset) over
// all queries q and all windows i that lie wholly inside the read, on back-to-back ASCII reads (reads_best_kernel) and on the packed words
// encode_fixed writes (reads_best_packed_kernel).
//
// Both layouts are one contiguous run of bases with a period P (ASCII: read_len; packed: 32 ceil(read_len / 32)): window j of the run belongs to read
// j div P and is admissible iff j mod P <= read_len - k.  The front end is the best match's, unchanged (scan_best_device.h: the block's tables in LDS,
// one wave-private strip per trip, AsciiStrip4 / PackedStrip4, grid.y = query blocks of kMultiQB queries); what is new is the back end, a SEGMENTED
// minimum.
//
// A lane's sixteen results of a round are windows of ONE segment of 32 (lane (n, h), register r: window 32 n + 8 (r >> 2) + 4 h + (r & 3)), and with
// P >= 32 a segment holds at most one read boundary: a lane sees at most two reads per round, A (the windows before the boundary) and B (those after
// it).  The accumulator's start values are a free additive term per (lane, register), so the classes are told apart INSIDE the product (A's rows carry
// the scale 2^4, as the best match's):
//   an admissible window of A starts at   2^23 + r              -> 2^23 + 16 d + r            (positive; bit patterns order like (d, r))
//   an admissible window of B starts at -(2^23 + 1023 - r)      -> -(2^23 + 1023 - 16 d - r)  (negative; LARGER bit patterns = smaller (d, r))
//   an inadmissible window starts at      2^23 + 1024 + r       -> above every admissible A, below every B as an unsigned number
// Every value is an integer below 2^24: exact.  An unsigned MINIMUM over the sixteen bit patterns is then A's best window and an unsigned MAXIMUM B's
// (eight v_min3_u32 and eight v_max3_u32); no result is compared with its admissibility afterwards.  The start values depend on the round, not on the
// query: the round loop is OUTSIDE the query loop here (the LDS traffic is the same: B once per round and A per (round, query), instead of A once per
// trip and B per (round, query)), and a lane keeps (key, query) of A and of B over the block's queries -- a strict improvement of d only, so the
// lowest query and, the registers being in window order, the lowest offset survive.
//
// The end of a round: the lane's two results become 64-bit keys d << 58 | q << 32 | i and go by LDS atomic minimum into a wave-private table indexed
// by (read - the trip's first read); after the trip's rounds the wave sends each touched entry with ONE global atomicMin into keys[read] -- which the
// launcher sets to all-ones first in the same stream (graph-safe, no ticket; a minimum does not depend on arrival order: deterministic) -- so a batch
// of 150-base reads costs one global atomic per (read, query block) and a read that spans many trips one per (trip, query block).
// reads_finish_kernel writes query / pos / dist with vector stores; the all-ones key (no admissible window) gives UINT32_MAX, UINT32_MAX, 0xFF.
// Where the read of a window is needed per lane, the quotient is small (below 132): a float estimate and one correction step, no 64-bit division; the
// trip's own (first read, offset) advance by a constant stride.
//
// P < 32 (reads shorter than a segment) runs no rounds: every window takes the one-window-per-thread path, which also serves the windows in front of the
// rounds and behind the last whole one, with the same admissibility test and one global atomicMin per (window, query block).
// Invalid bytes (ASCII) are latched by the first query block only, as the best match does.
//
// The RUNNER-UP (bitnuc_reads_hdist_best2*): the smallest (distance, query, offset) over the queries other than the winner's.  One pass with atomics
// cannot give it: which query is excluded is known only when every wave has delivered, so a merge of per-wave (best, second) pairs is no minimum and
// would depend on the order of arrival.  It is a SECOND PASS of the same kernels in their exclusion form (the template flag EX): keys1[] of the first
// pass is an input, a lane takes the winners' queries of its two reads A and B from it once per round (two loads that hit L2: keys1 was just written)
// and an improvement counts only when the query is not that one -- a compare and a select per (round, query) --; the one-window-per-thread path tests
// the same per query.  keys1 has one spare all-ones entry (B of the run's last segment is read `count`) and keys2 lies right behind it.  An all-ones key's query field is above every
// query: nothing is excluded.  The second pass validates nothing (the first did).  reads_finish2_kernel writes both triples.  EX = false is the code
// above, instruction for instruction.
#pragma once
#include "device_prims.h"
#include "scan_best_device.h" // best_tables_kernel, best_tables_to_lds, best_key, kBestScale; the front ends and mfma_chain through it

namespace bitnuc_dev {

constexpr int kReadsTable = 132;                  // reads a trip of 4096 windows can touch at P >= 32: 4096 / 32 + 2, and two spare
constexpr uint32_t kReadsBias = 0x4B000000u;      // the bit pattern of 2^23
constexpr uint32_t kReadsNoA = kReadsBias + 1024; // at or above: no admissible window of A
constexpr uint32_t kReadsNoB = 0xCB000000u;       // the bit pattern of -2^23: at or below, no admissible window of B
constexpr int kReadsQueryBits = 32;               // key = d << 58 | q << 32 | i
constexpr unsigned kReadsMinPeriod = 32;          // below: no rounds

struct ReadsGeom {
    unsigned long long period; // P
    unsigned lim;              // read_len - k: the last admissible offset
    float rcp;                 // 1 / P
};

__device__ __forceinline__ unsigned long long reads_key(uint32_t d, unsigned q, unsigned i) {
    return best_key(d, ((unsigned long long)q << kReadsQueryBits) | i);
}
// a key's query; of the all-ones key 2^26 - 1, above every query
__device__ __forceinline__ uint32_t reads_key_query(unsigned long long key) {
    return (uint32_t)(key >> kReadsQueryBits) & ((1u << (kBestPosBits - kReadsQueryBits)) - 1u);
}

// t = a P + o for a quotient below 2^20: a float estimate is within one of it
__device__ __forceinline__ void reads_divmod(unsigned long long t, const ReadsGeom &g, unsigned &a, unsigned &o) {
    unsigned q = (unsigned)((float)t * g.rcp);
    long long rem = (long long)t - (long long)(q * g.period);
    if (rem < 0) --q, rem += (long long)g.period;
    else if (rem >= (long long)g.period) ++q, rem -= (long long)g.period;
    a = q;
    o = (unsigned)rem;
}

// The lane's segment starts at offset o of its read A: [0, ea) are A's admissible windows, [b, eb] B's (b = 32: no boundary in the segment)
struct ReadsSegment { unsigned ea, b, eb; };
__device__ __forceinline__ ReadsSegment reads_segment(unsigned o, const ReadsGeom &g) {
    ReadsSegment s;
    const unsigned long long left = g.period - o; // >= 1
    s.b = left < 32 ? (unsigned)left : 32u;
    const unsigned open = o <= g.lim ? g.lim - o + 1u : 0u; // (lim < 2^32 - 1: no overflow)
    s.ea = open < s.b ? open : s.b;
    s.eb = s.b + (g.lim < 32u ? g.lim : 32u);
    return s;
}

// where the accumulators start (the top of the file); li(r) = 8 (r >> 2) + 4 h + (r & 3) is register r's window of the segment
__device__ __forceinline__ f32x16 reads_acc_start(const ReadsSegment &s, unsigned hh) {
    f32x16 c0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned li = 8u * (unsigned)(r >> 2) + 4u * hh + (unsigned)(r & 3);
        const float fa = bitnuc_host::kPackBias + (float)r, fb = -(bitnuc_host::kPackBias + (float)(1023 - r)), fn = bitnuc_host::kPackBias + (float)(1024 + r);
        c0[r] = li < s.ea ? fa : (li >= s.b && li <= s.eb) ? fb : fn;
    }
    asm volatile("" : "+v"(c0));
    return c0;
}

// the smallest and the largest of a round's sixteen results as bit patterns
__device__ __forceinline__ void round_min_max(const f32x16 &acc, uint32_t &mn, uint32_t &mx) {
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float f = acc[i]; // (__float_as_uint on a copy: pack_distances' note)
        x[i] = __float_as_uint(f);
    }
    mn = min(min(x[0], x[1]), x[2]);
    mx = max(max(x[0], x[1]), x[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) {
        mn = min(min(mn, x[i]), x[i + 1]);
        mx = max(max(mx, x[i]), x[i + 1]);
    }
    mn = min(mn, x[15]);
    mx = max(mx, x[15]);
}

__device__ __forceinline__ void reads_table_clear(unsigned long long *table, unsigned lane) {
    for (unsigned i = lane; i < (unsigned)kReadsTable; i += 64) table[i] = kBestNoKey;
}

// One trip: every round against every query of the block, the lane's results into the wave's table, the table into keys[read0 ..].  The trip's first
// window is window off0 of read read0; read_b(u, B): round u's B operand.  EX: excl[] holds the first pass' keys, whose queries are left out per read.
template <int U, bool EX, class ReadB>
__device__ __forceinline__ void reads_trip(const BestTable *qtab, unsigned nq, unsigned q0, unsigned row, unsigned m, unsigned lane, unsigned long long read0,
                                           unsigned off0, const ReadsGeom &g, unsigned long long *table, unsigned long long *__restrict__ keys,
                                           const unsigned long long *__restrict__ excl, ReadB read_b) {
    const unsigned m32 = lane & 31u, hh = lane >> 5;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if ((unsigned)u >= m) break; // wave-uniform
        unsigned a, o;
        reads_divmod((unsigned long long)off0 + 1024u * (unsigned)u + 32u * m32, g, a, o);
        const ReadsSegment s = reads_segment(o, g);
        const f32x16 c0 = reads_acc_start(s, hh);
        i32x8 B[4];
        read_b(u, B);
        uint32_t ka = kReadsNoA, kb = kReadsNoB, qa = 0, qb = 0;
        uint32_t xa = 0, xb = 0; // EX: the block's query that A / B leaves out (none of the block's: at or above kMultiQB)
        if constexpr (EX) {
            xa = reads_key_query(excl[read0 + a]) - q0;
            xb = reads_key_query(excl[read0 + a + 1]) - q0; // (at most read `count`: the spare entry)
        }
#pragma unroll
        for (int qi = 0; qi < kMultiQB; ++qi) {
            if ((unsigned)qi < nq) { // wave-uniform
                i32x8 A[4];
                query_operand<4>(qtab[qi].w[row], A);
                uint32_t mn, mx;
                round_min_max(mfma_chain(A, B, c0, kBestScale), mn, mx);
                bool fa = (mn | 15u) < ka;  // d below A's best d
                bool fb = (mx & ~15u) > kb; // d below B's best d
                if constexpr (EX) {
                    fa = fa && xa != (uint32_t)qi;
                    fb = fb && xb != (uint32_t)qi;
                }
                ka = fa ? mn : ka;
                qa = fa ? (uint32_t)qi : qa;
                kb = fb ? mx : kb;
                qb = fb ? (uint32_t)qi : qb;
            }
        }
        if (ka < kReadsNoA) {
            const uint32_t x = ka & 0x7FFFFFu, r = x & 15u;
            atomicMin(table + a, reads_key(x >> kBestShift, q0 + qa, o + 8u * (r >> 2) + 4u * hh + (r & 3u)));
        }
        if (kb > kReadsNoB) {
            const uint32_t x = 1023u - (kb & 0x7FFFFFu), r = x & 15u;
            atomicMin(table + a + 1, reads_key(x >> kBestShift, q0 + qb, 8u * (r >> 2) + 4u * hh + (r & 3u) - s.b));
        }
    }
    wave_lds_fence(); // the lanes' minima are in the table
    unsigned last, lo;
    reads_divmod((unsigned long long)off0 + 1024u * m - 1u, g, last, lo);
    for (unsigned i = lane; i <= last; i += 64) {
        const unsigned long long v = table[i];
        if (v != kBestNoKey) {
            atomicMin(keys + read0 + i, v);
            table[i] = kBestNoKey;
        }
    }
}

// where a wave's trips start in read coordinates: trip t0 of the wave begins at window off of read `read`; advance() moves one grid stride on
struct ReadsCursor {
    unsigned long long read, dq;
    unsigned long long off, dr, period;
    __device__ __forceinline__ ReadsCursor(unsigned long long j0, unsigned long long stride, unsigned long long period)
        : read(j0 / period), dq(stride / period), off(j0 % period), dr(stride % period), period(period) {}
    __device__ __forceinline__ void advance() {
        read += dq;
        off += dr;
        if (off >= period) off -= period, ++read;
    }
};

// The windows [0, pre) and [first, n) of the run, one per thread of the grid's x extent, every query of the block: word_of(j) is window j's 2-bit word
// (read only for an admissible window: it lies inside its read); check(j) validates base j of the run -- the bases behind the last round that only
// windows of the rounds cover are seen by no window here.  EX: the query of excl[read] is left out.
template <bool EX, class Q, class WordOf, class Check>
__device__ __forceinline__ void reads_tail_windows(unsigned long long pre, unsigned long long first, unsigned long long n, unsigned k, const ReadsGeom &g,
                                                   const Q *__restrict__ queries, unsigned nq, unsigned q0, unsigned long long *__restrict__ keys,
                                                   const unsigned long long *__restrict__ excl, WordOf word_of, Check check) {
    const QueryKind<Q> kind(k);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (n > first ? n - first : 0);
    for (unsigned long long t = gt; t < total; t += nthreads) {
        const unsigned long long j = t < pre ? t : first + (t - pre);
        check(j);
        const unsigned long long read = j / g.period, off = j - read * g.period;
        if (off > g.lim) continue;
        const auto w = kind.window(word_of(j));
        unsigned long long key = kBestNoKey;
        uint32_t x = 0;
        if constexpr (EX) x = reads_key_query(excl[read]) - q0;
        for (unsigned qi = 0; qi < nq; ++qi) { // ascending queries: the lowest of equal distances stays
            const unsigned long long c = reads_key(kind.dist(w, queries[qi]), q0 + qi, (unsigned)off);
            if constexpr (EX) key = (c < key && qi != x) ? c : key;
            else key = c < key ? c : key;
        }
        if (!EX || key != kBestNoKey) atomicMin(keys + read, key);
    }
}

// a kernel's one keys argument: the keys it fills, and with EX the first pass' keys in front of them (count + 1 entries, the last a spare all-ones
// one; count = n / P)
template <bool EX> struct ReadsKeys {
    unsigned long long *out;
    const unsigned long long *excl;
    __device__ __forceinline__ ReadsKeys(unsigned long long *keys, unsigned long long n, const ReadsGeom &g) : out(keys), excl(nullptr) {
        if constexpr (EX) excl = keys, out = keys + n / g.period + 1;
    }
};

// keys[r] -> query[r], pos[r], dist[r] (dist at any byte offset)
__global__ void __launch_bounds__(256) reads_finish_kernel(const unsigned long long *__restrict__ keys, unsigned long long count, uint32_t *__restrict__ query,
                                                           uint32_t *__restrict__ pos, uint8_t *__restrict__ dist) {
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < count; r += nthreads) {
        const unsigned long long key = keys[r];
        const bool none = key == kBestNoKey;
        query[r] = none ? 0xFFFFFFFFu : (uint32_t)(key >> kReadsQueryBits) & ((1u << (kBestPosBits - kReadsQueryBits)) - 1u);
        pos[r] = none ? 0xFFFFFFFFu : (uint32_t)key;
        dist[r] = none ? (uint8_t)0xFF : (uint8_t)(key >> kBestPosBits);
    }
}

// the six outputs of the best and the runner-up: keys1[r] -> query[r], pos[r], dist[r]; keys2[r] -> query2[r], pos2[r], dist2[r]
__global__ void __launch_bounds__(256) reads_finish2_kernel(const unsigned long long *__restrict__ keys1, const unsigned long long *__restrict__ keys2,
                                                            unsigned long long count, uint32_t *__restrict__ query, uint32_t *__restrict__ pos,
                                                            uint8_t *__restrict__ dist, uint32_t *__restrict__ query2, uint32_t *__restrict__ pos2,
                                                            uint8_t *__restrict__ dist2) {
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < count; r += nthreads) {
        const unsigned long long k1 = keys1[r], k2 = keys2[r];
        const bool none1 = k1 == kBestNoKey, none2 = k2 == kBestNoKey;
        query[r] = none1 ? 0xFFFFFFFFu : reads_key_query(k1);
        pos[r] = none1 ? 0xFFFFFFFFu : (uint32_t)k1;
        dist[r] = none1 ? (uint8_t)0xFF : (uint8_t)(k1 >> kBestPosBits);
        query2[r] = none2 ? 0xFFFFFFFFu : reads_key_query(k2);
        pos2[r] = none2 ? 0xFFFFFFFFu : (uint32_t)k2;
        dist2[r] = none2 ? (uint8_t)0xFF : (uint8_t)(k2 >> kBestPosBits);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Back-to-back ASCII reads at any alignment: the rounds start at reads + skip (16-byte aligned); n = count * read_len, the period is read_len.
// rounds: the launcher's (scan_rounds(n, skip), or 0 below kReadsMinPeriod).  EX: the second pass -- keys[0, count] are the first pass' keys (the
// exclusion's input) and the keys it fills lie behind them, from keys + count + 1 (no further argument: the argument block of EX = false stays the
// best match's); nothing is validated and slot is unused.
template <int U, bool EX, class Q>
__global__ void __launch_bounds__(kMultiBlock)
reads_best_kernel(const uint8_t *__restrict__ ref, unsigned long long n, unsigned skip, unsigned long long rounds, unsigned k, const ReadsGeom g,
                  const Q *__restrict__ queries, unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys,
                  unsigned long long *__restrict__ slot) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][AsciiStrip4<U>::kBytes];
    __shared__ unsigned long long tables[kMultiBlock / 64][kReadsTable];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    const bool latch = !EX && blockIdx.y == 0; // one query block reports invalid bytes
    best_tables_to_lds(tabs + q0, nq, qtab);
    const ReadsKeys<EX> kk(keys, n, g);

    const uint8_t *base = ref + skip;
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const AsciiStrip4<U> fe(strips[wave_in_block()], lane);
    unsigned long long *table = tables[wave_in_block()];
    reads_table_clear(table, lane);

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) {
        scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
        ReadsCursor at(skip + (r0 << 10), (nwaves * U) << 10, g.period);
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
            reads_trip<U, EX>(qtab, nq, q0, fe.row, m, lane, at.read, (unsigned)at.off, g, table, kk.out, kk.excl, [&](int u, i32x8 (&B)[4]) { fe.read_b(u, B); });
            at.advance();
            r0 = rn;
        }
    }

    const unsigned long long pre = skip < n ? skip : n, first = skip + (rounds << 10);
    reads_tail_windows<EX>(pre, first, n, k, g, queries + q0, nq, q0, kk.out, kk.excl, [&](unsigned long long j) { return ascii_window_word(ref, j, k, false, slot); },
                           [&](unsigned long long j) { if (latch && !valid_base(ref[j])) latch_bad(slot, j, ref[j]); });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The packed words of encode_fixed (8-byte aligned; at 8 mod 16 the rounds start one word later): n = 32 * count * ceil(read_len / 32) bases, the period
// is 32 * ceil(read_len / 32).  The pad bits above a read's last base only ever reach inadmissible windows.
template <bool EX, class Q>
__global__ void __launch_bounds__(kMultiBlock)
reads_best_packed_kernel(const uint64_t *__restrict__ words, unsigned long long n, unsigned skip, unsigned long long rounds, unsigned k, const ReadsGeom g,
                         const Q *__restrict__ queries, unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][PackedStrip4::kBytes];
    __shared__ unsigned long long tables[kMultiBlock / 64][kReadsTable];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    best_tables_to_lds(tabs + q0, nq, qtab);
    const ReadsKeys<EX> kk(keys, n, g);

    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    uint8_t *strip = strips[wave_in_block()];
    const PackedStrip4 fe(strip, lane);
    unsigned rd[4]; // (here and not in fe: read_offsets' note)
    fe.read_offsets(rd);
    unsigned long long *table = tables[wave_in_block()];
    reads_table_clear(table, lane);

    unsigned long long r0 = wave * 4;
    if (r0 < rounds) {
        PackedTrip cur;
        packed_trip_load(base, r0, rounds, lane, cur);
        ReadsCursor at(skip + (r0 << 10), (nwaves * 4) << 10, g.period);
        while (r0 < rounds) {
            const unsigned m = trip_rounds(r0, rounds, 4u);
            const unsigned long long rn = r0 + nwaves * 4;
            wave_lds_fence(); // the previous trip's readers are done
            fe.fill(lane, m, cur);
            if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
            wave_lds_fence();
            reads_trip<4, EX>(qtab, nq, q0, fe.row, m, lane, at.read, (unsigned)at.off, g, table, kk.out, kk.excl, [&](int u, i32x8 (&B)[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) B[j] = PackedStrip4::operand(strip, rd[j], u);
            });
            at.advance();
            r0 = rn;
        }
    }

    const unsigned long long pre = skip < n ? skip : n, first = skip + (rounds << 10);
    reads_tail_windows<EX>(pre, first, n, k, g, queries + q0, nq, q0, kk.out, kk.excl, [&](unsigned long long j) { return packed_window_word(words, j, k); },
                           [](unsigned long long) {});
}

} // namespace bitnuc_dev
