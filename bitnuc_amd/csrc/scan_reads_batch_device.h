// scan_reads_batch_device.h -- the best match per READ of a RAGGED batch: scan_reads_device.h's result (for every read the lexicographically smallest
// (distance, query, offset) over all queries and all windows wholly inside the read) where the reads lie behind an offsets table instead of at one
// period: back-to-back ASCII reads (reads_batch_kernel: read r is seq[offsets[r], offsets[r + 1])) and the words encode_batch writes
// (reads_batch_packed_kernel: read r's ceil(len_r / 32) words start at words[word_offsets[r]]).
//
// Both layouts are one contiguous run of bases; read r STARTS at start_r (ASCII: offsets[r]; packed: 32 word_offsets[r]) and owns the windows up to
// start_(r + 1) -- its period, len_r on ASCII and 32 ceil(len_r / 32) on packed words -- of which those at offsets <= len_r - k are admissible.  Window
// j belongs to the LAST read with start_r <= j: an empty read owns nothing (on packed words it vanishes from the run) and never is that read.  The front
// end, the per-query tables, the product, the start values that tell A's, B's and inadmissible windows apart inside it, the segmented min / max, the
// 64-bit key, the wave's key table with its flush and reads_finish_kernel are scan_reads_device.h's, unchanged.  What is new is where a lane's segment
// lies:
//
//   per trip (4096 windows from j0), once per wave: the trip's first read by a wave-uniform 64-ary search of the table (each step 64 lanes probe 64
//   evenly spaced entries and a ballot keeps one 64th: four steps for 16 M reads), then the SLICE of the table the trip can touch, kReadsTable + 1
//   entries from that read, into wave-private LDS in the trip's own coordinates: entry i = (start_i - j0, adm_i - j0), adm_i = start_i + len_i - k + 1
//   the first window of read i that is NOT admissible -- both clamped to [0, 65535] (a trip ends at 4096: whatever is clamped lies before the trip or
//   behind it, which is all a lane needs to know), 4 bytes per entry.
//
//   per round, per lane: A = the last slice entry that starts at or before the segment (a binary search of the slice in LDS, eight reads), the boundary
//   b = min(32, start_(A + 1) - segment), A's admissible windows [0, min(b, adm_A - segment)), and -- only where the boundary is inside the segment --
//   B = the entry that owns the windows behind it: the LAST entry starting there (empty reads between A and B share B's start and are stepped over: B's
//   table entry is its own read index, not A + 1), with B's admissible windows [b, min(32, adm_B - segment)).  That is reads_segment with A's own
//   limit (len_A - k, which may be negative: adm_A at or before start_A), B's own limit and A's own period, in trip coordinates.
//
// A segment of 32 windows holds at most ONE boundary only where every read it touches owns at least 32 windows.  Packed: every non-empty read does.
// ASCII: a read of 1 .. 31 bases does not, and the slice cannot hold a trip that touches more than kReadsTable reads (empty reads count: they take an
// entry without taking windows).  So per trip the wave marks the ROUNDS that touch a read owning fewer than 32 windows (all of them when the slice
// overflows); a marked round runs no product: its 1024 windows take the exact one-window-per-thread path (batch_exact_window: the read by a galloping
// search of the table from the trip's first read, the distance by popcount, one global atomicMin per (window, query block)), which also serves the
// windows in front of the rounds and behind the last whole one.  Same keys, same minimum: the same result whichever path a window takes.
//
// Which batches run at full speed: packed words always, unless a trip touches more than kReadsTable reads (more than 128 one-word reads plus empty
// ones); ASCII wherever a round of 1024 windows touches no read of 1 .. 31 bases.  A batch of such short reads runs wholly on the exact path.
//
// Atomics: one global atomicMin per (read, query block) and trip on the fast path, as the fixed-length form.  The keys are preset to all-ones in-stream,
// so an empty read, or one shorter than k, is filled by reads_finish_kernel with no code of its own.  The tables are read at every launch: a replayed
// graph sees the lengths of the replay.  Invalid bytes (ASCII) are latched by the first query block only.
#pragma once
#include "scan_reads_device.h"

namespace bitnuc_dev {

constexpr unsigned kBatchFar = 0xFFFFu;  // a slice coordinate at or beyond this is "behind the trip"
constexpr unsigned kBatchMinOwn = 32;    // a read that owns fewer windows (and at least one) sends its rounds to the exact path

// The layout's tables as the kernels read them: starts[r] << shift is read r's first window of the run (ASCII: offsets, 0; packed: word_offsets, 5),
// offsets the base offsets (the lengths).  count + 1 entries each.
struct BatchTables {
    const unsigned long long *__restrict__ starts;
    const unsigned long long *__restrict__ offsets;
    unsigned long long count;
    unsigned shift;
    __device__ __forceinline__ unsigned long long start(unsigned long long r) const { return starts[r] << shift; }
    __device__ __forceinline__ unsigned long long len(unsigned long long r) const { return offsets[r + 1] - offsets[r]; }
};

// the last read r with start(r) <= j, wave-uniform (start(0) = 0 <= j < start(count)): every step keeps one 64th of [lo, hi)
__device__ __forceinline__ unsigned long long batch_first_read(const BatchTables &t, unsigned long long j, unsigned lane) {
    unsigned long long lo = 0, hi = t.count;
    while (hi - lo > 1) {
        const unsigned long long step = (hi - lo + 63) >> 6;
        const unsigned long long p = lo + step * lane;
        const bool le = p < hi && t.start(p) <= j; // a prefix of the lanes (the table does not decrease); lane 0 always
        const unsigned c = (unsigned)__builtin_popcountll(__ballot(le));
        lo += step * (unsigned long long)(c ? c - 1u : 0u);
        hi = lo + step < hi ? lo + step : hi;
    }
    return lo;
}

// where a trip lies: its first read, the trip's first window as an offset into that read, and the rounds that take the exact path (bit u)
struct BatchTrip {
    unsigned long long read0, off0;
    unsigned exact;
};

// The trip's slice into LDS (the top of the file); the trip is the m rounds from window j0.
__device__ __forceinline__ BatchTrip batch_trip_locate(const BatchTables &t, unsigned long long j0, unsigned m, unsigned k, unsigned lane, uint32_t *slice) {
    BatchTrip trip;
    trip.read0 = batch_first_read(t, j0, lane);
    trip.off0 = j0 - t.start(trip.read0);
    const long long end = 1024ll * m;
    unsigned mine = 0; // the rounds this lane's entries send to the exact path
    for (unsigned i = lane; i <= (unsigned)kReadsTable; i += 64) {
        const unsigned long long idx = trip.read0 + i;
        unsigned srel = kBatchFar, adm = 0;
        if (idx <= t.count) {
            const unsigned long long s = t.start(idx);
            const long long d = (long long)(s - j0); // i >= 1: positive
            srel = i == 0 ? 0u : d < (long long)kBatchFar ? (unsigned)d : kBatchFar;
            if (i == (unsigned)kReadsTable && d < end) mine = 15u; // a read the slice does not hold starts inside the trip
            if (idx < t.count) {
                const long long a = (long long)(s + t.len(idx)) - (long long)k + 1 - (long long)j0;
                adm = a <= 0 ? 0u : a < (long long)kBatchFar ? (unsigned)a : kBatchFar;
                const long long own = (long long)(t.start(idx + 1) - s);
                if (own > 0 && own < (long long)kBatchMinOwn && d < end) { // (own < 32: the read ends after the trip's start)
                    const unsigned u0 = d > 0 ? (unsigned)(d >> 10) : 0u;
                    const long long last = d + own - 1 < end - 1 ? d + own - 1 : end - 1;
                    const unsigned u1 = (unsigned)(last >> 10);
                    mine |= ((2u << u1) - 1u) & ~((1u << u0) - 1u);
                }
            }
        }
        slice[i] = adm << 16 | srel;
    }
    trip.exact = 0;
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) trip.exact |= __ballot((mine >> u) & 1u) != 0ull ? 1u << u : 0u;
    return trip;
}

// the last of the slice's kReadsTable reads that starts at or before window w of the trip (entry 0 does; eight halvings).  Entry kReadsTable is only
// ever a read's END: where it starts inside the trip every round is exact and nothing is looked up.
__device__ __forceinline__ unsigned batch_slice_find(const uint32_t *slice, unsigned w) {
    unsigned lo = 0, hi = (unsigned)kReadsTable;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const unsigned mid = (lo + hi) >> 1;
        const bool le = (slice[mid] & 0xFFFFu) <= w; // (mid == lo: true, nothing moves)
        lo = le ? mid : lo;
        hi = le ? hi : mid;
    }
    return lo;
}
static_assert(kReadsTable <= 256, "batch_slice_find halves eight times");

// The lane's segment starts at window w of the trip: reads_segment with A's and B's own limits and A's own period, from the slice.  a / b: the two
// reads' slice entries (b only where the boundary is inside the segment), oa: the segment's offset into A less the trip's (entry 0: add the trip's off0).
struct BatchSegment {
    ReadsSegment s;
    unsigned a, b, oa;
};
__device__ __forceinline__ BatchSegment batch_segment(const uint32_t *slice, unsigned w) {
    BatchSegment g;
    g.a = batch_slice_find(slice, w);
    const uint32_t ea = slice[g.a];
    const unsigned next = slice[g.a + 1] & 0xFFFFu; // > w
    g.oa = w - (ea & 0xFFFFu);
    g.s.b = next - w < 32u ? next - w : 32u;
    const int open = (int)(ea >> 16) - (int)w;
    g.s.ea = open <= 0 ? 0u : (unsigned)open < g.s.b ? (unsigned)open : g.s.b;
    g.b = g.a + 1;
    g.s.eb = g.s.b - 1u; // no window of B
    if (g.s.b < 32u) {
        while (g.b + 1u < (unsigned)kReadsTable && (slice[g.b + 1] & 0xFFFFu) == next) ++g.b; // over the empty reads that start where B does
        int last = (int)(slice[g.b] >> 16) - (int)w - 1;
        last = last < 31 ? last : 31;
        if (last >= (int)g.s.b) g.s.eb = (unsigned)last;
    }
    return g;
}

// One window of the run on the exact path, every query of the block: the read by a galloping search from `from` (start(from) <= j), then
// reads_tail_windows' body.  word_of(j) is read only for an admissible window.
template <class Q, class WordOf>
__device__ __forceinline__ void batch_exact_window(const BatchTables &t, unsigned long long j, unsigned long long from, const QueryKind<Q> &kind, unsigned k,
                                                   const Q *__restrict__ queries, unsigned nq, unsigned q0, unsigned long long *__restrict__ keys, WordOf word_of) {
    unsigned long long lo = from, hi = from + 1, step = 1;
    while (hi < t.count && t.start(hi) <= j) lo = hi, hi += step, step <<= 1;
    hi = hi < t.count ? hi : t.count;
    while (hi - lo > 1) { // start(lo) <= j < start(hi)
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (t.start(mid) <= j) lo = mid;
        else hi = mid;
    }
    const unsigned long long off = j - t.start(lo), len = t.len(lo);
    if (off + k > len) return;
    const auto w = kind.window(word_of(j));
    unsigned long long key = kBestNoKey;
    for (unsigned qi = 0; qi < nq; ++qi) { // ascending queries: the lowest of equal distances stays
        const unsigned long long c = reads_key(kind.dist(w, queries[qi]), q0 + qi, (unsigned)off);
        key = c < key ? c : key;
    }
    atomicMin(keys + lo, key);
}

// One trip: reads_trip with the lane's segment from the slice; the rounds marked exact run afterwards, one window per lane at a time.
template <int U, class Q, class ReadB, class WordOf>
__device__ __forceinline__ void batch_trip(const BestTable *qtab, unsigned nq, unsigned q0, unsigned row, unsigned m, unsigned lane, const BatchTables &t,
                                           unsigned long long j0, const BatchTrip &trip, const uint32_t *slice, unsigned long long *table, unsigned k,
                                           const Q *__restrict__ queries, unsigned long long *__restrict__ keys, ReadB read_b, WordOf word_of) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if ((unsigned)u >= m) break;          // wave-uniform
        if ((trip.exact >> u) & 1u) continue; // wave-uniform
        // (the lane's column and K-block from the hardware lane id, per round, and both query indices in one register below: held across the trip in
        // registers of their own they cost the kernels 20 / 28 bytes of scratch per lane, with a reload in front of every round's MFMA chain)
        const unsigned l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), m32 = l & 31u, hh = l >> 5;
        const BatchSegment g = batch_segment(slice, 1024u * (unsigned)u + 32u * m32);
        const f32x16 c0 = reads_acc_start(g.s, hh);
        i32x8 B[4];
        read_b(u, B);
        uint32_t ka = kReadsNoA, kb = kReadsNoB, qab = 0; // qab: A's query in the low half, B's in the high
#pragma unroll
        for (int qi = 0; qi < kMultiQB; ++qi) {
            if ((unsigned)qi < nq) { // wave-uniform
                i32x8 A[4];
                query_operand<4>(qtab[qi].w[row], A);
                uint32_t mn, mx;
                round_min_max(mfma_chain(A, B, c0, kBestScale), mn, mx);
                const bool fa = (mn | 15u) < ka;  // d below A's best d
                const bool fb = (mx & ~15u) > kb; // d below B's best d
                ka = fa ? mn : ka;
                qab = fa ? (qab & 0xFFFF0000u) | (uint32_t)qi : qab;
                kb = fb ? mx : kb;
                qab = fb ? (qab & 0xFFFFu) | ((uint32_t)qi << 16) : qab;
            }
        }
        if (ka < kReadsNoA) {
            const uint32_t x = ka & 0x7FFFFFu, r = x & 15u;
            const unsigned o = g.oa + (g.a == 0 ? (unsigned)trip.off0 : 0u); // (admissible: below 2^32)
            atomicMin(table + g.a, reads_key(x >> kBestShift, q0 + (qab & 0xFFFFu), o + 8u * (r >> 2) + 4u * hh + (r & 3u)));
        }
        if (kb > kReadsNoB) {
            const uint32_t x = 1023u - (kb & 0x7FFFFFu), r = x & 15u;
            atomicMin(table + g.b, reads_key(x >> kBestShift, q0 + (qab >> 16), 8u * (r >> 2) + 4u * hh + (r & 3u) - g.s.b));
        }
    }
    wave_lds_fence(); // the lanes' minima are in the table
    for (unsigned i = lane; i < (unsigned)kReadsTable; i += 64) {
        const unsigned long long v = table[i];
        if (v != kBestNoKey) { // (an admissible window's: a read of the batch)
            atomicMin(keys + trip.read0 + i, v);
            table[i] = kBestNoKey;
        }
    }
    if (__builtin_expect(trip.exact != 0u, 0)) {
        const QueryKind<Q> kind(k);
#pragma unroll 1
        for (unsigned u = 0; u < m; ++u) {
            if (!((trip.exact >> u) & 1u)) continue;
#pragma unroll 1
            for (unsigned w = 1024u * u + lane; w < 1024u * (u + 1u); w += 64)
                batch_exact_window(t, j0 + w, trip.read0, kind, k, queries, nq, q0, keys, word_of);
        }
    }
}

// the windows [0, pre) and [first, n) of the run, one per thread of the grid's x extent (reads_tail_windows on a table); check(j) validates base j
template <class Q, class WordOf, class Check>
__device__ __forceinline__ void batch_tail_windows(const BatchTables &t, unsigned long long pre, unsigned long long first, unsigned long long n, unsigned k,
                                                   const Q *__restrict__ queries, unsigned nq, unsigned q0, unsigned long long *__restrict__ keys,
                                                   WordOf word_of, Check check) {
    const QueryKind<Q> kind(k);
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long total = pre + (n > first ? n - first : 0);
    for (unsigned long long i = gt; i < total; i += nthreads) {
        const unsigned long long j = i < pre ? i : first + (i - pre);
        check(j);
        batch_exact_window(t, j, 0, kind, k, queries, nq, q0, keys, word_of);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Back-to-back ASCII reads at any alignment: the rounds start at seq + skip (16-byte aligned); n = offsets[count] >= 1, rounds = scan_rounds(n, skip).
template <int U, class Q>
__global__ void __launch_bounds__(kMultiBlock)
reads_batch_kernel(const uint8_t *__restrict__ ref, const BatchTables t, unsigned long long n, unsigned skip, unsigned long long rounds, unsigned k,
                   const Q *__restrict__ queries, unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys,
                   unsigned long long *__restrict__ slot) {
    static_assert(U == 4, "a trip's exact-round mask has four bits");
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][AsciiStrip4<U>::kBytes];
    __shared__ unsigned long long tables[kMultiBlock / 64][kReadsTable];
    __shared__ uint32_t slices[kMultiBlock / 64][kReadsTable + 1];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    const bool latch = blockIdx.y == 0; // one query block reports invalid bytes
    best_tables_to_lds(tabs + q0, nq, qtab);

    const uint8_t *base = ref + skip;
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    const AsciiStrip4<U> fe(strips[wave_in_block()], lane);
    unsigned long long *table = tables[wave_in_block()];
    uint32_t *slice = slices[wave_in_block()];
    reads_table_clear(table, lane);
    const auto word_of = [&](unsigned long long j) { return ascii_window_word(ref, j, k, false, slot); };

    ScanTrip<U> cur;
    unsigned long long r0 = wave * U;
    if (r0 < rounds) {
        scan_trip_load<U, 3, true>(base, r0, rounds, lane, cur);
        while (r0 < rounds) {
            const unsigned m = trip_rounds(r0, rounds, U);
            const unsigned long long rn = r0 + nwaves * U, j0 = skip + (r0 << 10);
            wave_lds_fence(); // the previous trip's readers are done
            const BatchTrip trip = batch_trip_locate(t, j0, m, k, lane, slice);
            const uint32_t trip_bad = fe.fill(lane, m, cur);
            if (latch && __builtin_expect(trip_invalid(trip_bad), 0)) {
#pragma unroll 1
                for (unsigned u = 0; u < m; ++u) rescan_bytes(ref, skip + ((r0 + u) << 10) + 16 * lane, 16, slot);
            }
            if (rn < rounds) scan_trip_load<U, 3, true>(base, rn, rounds, lane, cur); // cur's bytes are in the strip: its registers take the next trip
            wave_lds_fence();
            batch_trip<U>(qtab, nq, q0, fe.row, m, lane, t, j0, trip, slice, table, k, queries + q0, keys, [&](int u, i32x8 (&B)[4]) { fe.read_b(u, B); }, word_of);
            r0 = rn;
        }
    }

    const unsigned long long pre = skip < n ? skip : n, first = skip + (rounds << 10);
    batch_tail_windows(t, pre, first, n, k, queries + q0, nq, q0, keys, word_of,
                       [&](unsigned long long j) { if (latch && !valid_base(ref[j])) latch_bad(slot, j, ref[j]); });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The packed words of encode_batch (8-byte aligned; at 8 mod 16 the rounds start one word later): n = 32 * word_offsets[count] >= 32.  The pad bits
// above a read's last base only ever reach inadmissible windows.
template <class Q>
__global__ void __launch_bounds__(kMultiBlock)
reads_batch_packed_kernel(const uint64_t *__restrict__ words, const BatchTables t, unsigned long long n, unsigned skip, unsigned long long rounds, unsigned k,
                          const Q *__restrict__ queries, unsigned n_queries, const BestTable *__restrict__ tabs, unsigned long long *__restrict__ keys) {
    __shared__ __attribute__((aligned(16))) BestTable qtab[kMultiQB];
    __shared__ __attribute__((aligned(16))) uint8_t strips[kMultiBlock / 64][PackedStrip4::kBytes];
    __shared__ unsigned long long tables[kMultiBlock / 64][kReadsTable];
    __shared__ uint32_t slices[kMultiBlock / 64][kReadsTable + 1];
    const unsigned q0 = blockIdx.y * kMultiQB;
    const unsigned nq = n_queries - q0 < (unsigned)kMultiQB ? n_queries - q0 : (unsigned)kMultiQB;
    best_tables_to_lds(tabs + q0, nq, qtab);

    const uint8_t *base = reinterpret_cast<const uint8_t *>(words + (skip >> 5));
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + wave_in_block();
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    uint8_t *strip = strips[wave_in_block()];
    const PackedStrip4 fe(strip, lane);
    unsigned rd[4]; // (here and not in fe: read_offsets' note)
    fe.read_offsets(rd);
    unsigned long long *table = tables[wave_in_block()];
    uint32_t *slice = slices[wave_in_block()];
    reads_table_clear(table, lane);
    const auto word_of = [&](unsigned long long j) { return packed_window_word(words, j, k); };

    unsigned long long r0 = wave * 4;
    if (r0 < rounds) {
        PackedTrip cur;
        packed_trip_load(base, r0, rounds, lane, cur);
        while (r0 < rounds) {
            const unsigned m = trip_rounds(r0, rounds, 4u);
            const unsigned long long rn = r0 + nwaves * 4, j0 = skip + (r0 << 10);
            wave_lds_fence(); // the previous trip's readers are done
            const BatchTrip trip = batch_trip_locate(t, j0, m, k, lane, slice);
            fe.fill(lane, m, cur);
            if (rn < rounds) packed_trip_load(base, rn, rounds, lane, cur); // cur's bases are in the strip: its registers take the next trip
            wave_lds_fence();
            batch_trip<4>(qtab, nq, q0, fe.row, m, lane, t, j0, trip, slice, table, k, queries + q0, keys, [&](int u, i32x8 (&B)[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) B[j] = PackedStrip4::operand(strip, rd[j], u);
            }, word_of);
            r0 = rn;
        }
    }

    const unsigned long long pre = skip < n ? skip : n, first = skip + (rounds << 10);
    batch_tail_windows(t, pre, first, n, k, queries + q0, nq, q0, keys, word_of, [](unsigned long long) {});
}

} // namespace bitnuc_dev
