// scan_anchored_device.h -- the ANCHORED best match and runner-up per read (bitnuc_reads_hdist_anchored*): the smallest (distance, query, offset) over
// Q queries and the offsets pos_lo .. hi_eff of every read of a fixed-length batch, and the smallest over the queries other than the winner's.
//
// Not a sliding product.  The sliding kernels (scan_reads_device.h) make a column of 32 consecutive windows of ONE long sequence and a row of a shift of
// ONE query: their operand is a Toeplitz band of the query, and a read's few admissible windows would be a sliver of every tile.  With an offset range
// the question is a plain GEMM: dist[r][(q, s)] = k - sum_p onehot(read_r[pos_lo + p]) . onehot(q[p - s]) over the span's positions p < span <= 64.
//   B (columns): 32 reads; K = the span's positions x 4 channels (16 bases per K-step of 64 fp4 nibbles, a base's nibbles A, C, G, T side by side).
//   A (rows):    32 (query, shift) pairs: the query's one-hot, as -1.0 (fp4 0b1010), at positions s .. s + k - 1, zero elsewhere, with the E8M0 scale 2^17.
//   D:           lane l holds column l & 31 = ONE READ; its 16 registers and those of lane l ^ 32 are that read's 32 rows (scan_mfma_device.h, top).
// The accumulators start at 2^23 + (k << 17) + local, so a result's bit pattern is 0x4B000000 | dist << 17 | local and an unsigned minimum over patterns
// is the smallest (distance, local).  Rows are ordered query-major: every query owns P = 2^lg >= offsets rows (rows with s >= offsets, and the rows
// behind the last query, have an all-zero A and start at 63 << 17: no real row can beat them).  The row of register r in K-block half h is given the
// slot 16 h + r, so for P <= 16 a query's shifts are P consecutive registers of one lane: minimum over the shifts, then a top-2 over the lane's queries
// with min / max only (they are distinct), two keys made global (dist << 26 | q P + s) and merged into the lane's running (best, second).  The two
// lanes of a read hold different queries and merge once, after the last tile.  P = 32 (64): a query is a whole tile (two): one v_permlane32_swap per tile
// joins the halves, both lanes keep the same state.  No atomics, no key arrays, no finish kernel: lane l < 32 writes its read's six outputs itself.
//
// Operand path: REGISTERS, no LDS strip.  In the sliding kernels a lane's loaded bytes are other lanes' operands, hence the strip; here lane (n, h) needs
// bases 16 j + 8 h .. + 8 of its OWN read's span, so it loads exactly those: the aligned dwords that hold them (nothing outside a dword that holds a span
// byte is touched), v_alignbyte to the piece, onehot8 + two v_perm to interleave.  (Up to three 4-byte loads per piece at the reads' stride instead
// of the 16-byte aligned gathers of the batch kernels: NOT A/B'd against them; a likely part of why the ASCII form reaches 0.38 - 0.50 of the memory floor.)  Packed: the word (or two) that holds the piece's 16 bits, a funnel
// shift, the codes spread to bytes and scan_packed_device.h's two LUTs.  A wave keeps the operands of TWO groups of 32 reads (64 reads) and walks the
// query tiles once for both: a tile's A operand is four 16-byte loads per lane from a per-query table in context scratch (256 bytes per query: the
// query's one-hot at entries 64 .. 64 + k - 1 of 128, so that every shift of every K-step is one unaligned 16-byte piece of it; built in-stream by
// anchored_tables_kernel, L2-resident), and with two groups those 4 KiB feed eight matrix instructions instead of four.
// Pattern queries (a set of bases per position, bitnuc_reads_pattern_anchored*) differ in the table alone: an entry holds -1.0 in every channel of its
// position's set (anchored_entry), the kernel below is the same instantiations.
// Channels: four per base (16 bases per K-step, ceil(span / 16) MFMAs per tile and group).  Three channels (T = 0, 21 bases per K-step) would save one
// MFMA of four at spans of 49 .. 63 and one of two at 17 .. 21, at the price of a second table and operand form; not shipped.
// Invalid ASCII bytes: ascii_residue's LUT on every piece, restricted to the span's bytes; a lane that sees one latches its first (atomicMin: the first
// in buffer order wins).
//
// Two layouts, one kernel (the template parameter G, everything that differs under `if constexpr`).  Fixed (AnchorGeom): reads at a stride, one range for
// all of them -- the text above.  RAGGED (AnchorBatchGeom, bitnuc_reads_hdist_anchored_batch*): reads behind an offsets table, the range counted from each
// read's start or from its end.  A lane already is one read, so the layout is per-lane data: the lane loads its read's two table entries (coalesced) and
// derives a_r, the offset of row 0, and n_r <= offsets, its number of admissible offsets (anchored_lane); its pieces are cut at n_r + k - 1 bytes, so
// nothing behind its own span is loaded or validated; row s is offset a_r + s.  The A operand is shared by the tile's 32 reads, so a row that one read
// does not admit is live for its neighbours: admissibility is per (row, column) and sits in the accumulators' START VALUES (a lane holds one column),
// computed once per block and group for the tiles whose queries all exist -- the tile loop is the fixed layout's, instruction for instruction apart from
// constants.  A live inadmissible row collects matches, so its start value must stay out of reach of 32 of them: the ragged layout widens the distance
// field to seven bits (AnchorField).  The fixed instantiations' instructions are those of the kernel before it had a second layout.
#pragma once
#include "device_prims.h"
#include "scan_mfma_device.h"   // i32x8, f32x16, onehot8, dword_residue, trip_invalid
#include "scan_packed_device.h" // lut_ac, lut_gt

namespace bitnuc_dev {

constexpr int kAnchorBlock = 256;          // four waves, nothing shared between them
constexpr int kAnchorGroups = 2;           // groups of 32 reads per wave and tile walk
constexpr unsigned kAnchorEntry = 256;     // bytes of a query's table entry: 128 bases x 16 bits
constexpr uint32_t kAnchorBias = 0x4B000000u; // 2^23

// stride: bytes (ASCII) or words (packed) per read; lg: log2 of the rows per query; ntiles: ceil(nq << lg / 32)
struct AnchorGeom { unsigned long long stride; unsigned pos_lo, span, offsets, lg, k, nq, ntiles; static constexpr bool kRagged = false; };

// The RAGGED layout (bitnuc_reads_hdist_anchored_batch*), the kernel's other layout policy: read r is tab[r] .. tab[r + 1] (bytes of ASCII, bases of packed
// words that start at word wtab[r]); the range is pos_lo .. pos_lo + offsets - 1, counted from the read's start or (end != 0) in bases BEHIND the window.
// span = offsets + k - 1 is the widest span; every read has its own first span base a_r and number of admissible offsets n_r <= offsets (AnchorLane).
struct AnchorBatchGeom {
    const unsigned long long *tab, *wtab;
    unsigned pos_lo, end, span, offsets, lg, k, nq, ntiles;
    static constexpr bool kRagged = true;
};

// The distance field of an accumulator's bit pattern.  Fixed layout: six bits at bit 17, an inadmissible row starts at 63 and has an all-zero A, so it
// stays there.  Ragged: a row that is inadmissible for one read of the tile is admissible for its neighbours and has a LIVE A -- up to 32 matches would
// take 63 down to 31, a real distance --, so the field is seven bits at bit 16 (bits 6 .. 16 were unused) and such a row starts at 127: it ends at 95 or
// above, no real distance (<= 32) and behind every real row in the unsigned minimum.  Costs nothing in the tile loop: only constants differ.
// Pattern queries (bitnuc_reads_pattern_anchored*): an entry may hold -1.0 in several channels, but B has ONE non-zero nibble per read base, so a
// position still subtracts at most 1 << kShift and a row at most k <= 32 of them: the same bound.  An all-N pattern at k = 32 matches at every position
// of every read, so its live inadmissible rows end at exactly 127 - 32 = 95: the bound is reached, not exceeded (tests/test_gpu_reads_pattern.py).
// Bases behind a short read's span read as 'A' (anchored_piece_ascii, _packed) and match like any other: they are counted in the 32.
template <bool RAGGED> struct AnchorField {
    static constexpr unsigned kShift = RAGGED ? 16u : 17u;        // a match subtracts 1 << kShift
    static constexpr unsigned kNone = RAGGED ? 127u : 63u;        // where an inadmissible row starts
    static constexpr unsigned kKeyShift = RAGGED ? 25u : 26u;     // the field's place in a global key
    static constexpr uint32_t kKeyMask = ~0u << kKeyShift;
    static constexpr int kScale = 127 + (int)kShift;              // A's E8M0 scale
};

// position d < k of a query as a table entry: -1.0 (fp4 0b1010) in the nibble of every channel (A, C, G, T from bit 0) the query takes there.  An exact
// query: its base's one nibble.  A pattern (read as four dwords): the channels c whose allow[c] has bit d set -- B is one-hot, so the product of a
// position is -[base in S_d] and a position matches at most once; an empty set is an all-zero entry.  Bits of allow[c] at positions >= k are never
// looked at (the caller's d < k), d = 31 is an unsigned shift.
__device__ __forceinline__ uint32_t anchored_entry(unsigned long long q, unsigned d) { return 0xAu << (4u * (unsigned)((q >> (2u * d)) & 3u)); }
__device__ __forceinline__ uint32_t anchored_entry(const PatternSets &p, unsigned d) {
    uint32_t v = 0;
#pragma unroll
    for (unsigned c = 0; c < 4; ++c) v |= ((p.allow[c] >> d) & 1u) * (0xAu << (4u * c));
    return v;
}

// entry i of query q: position i - 64 of the query (anchored_entry), zero outside [0, k).  Q: the query kind (QueryKind, scan_mfma_device.h)
template <class Q>
__global__ void __launch_bounds__(64) anchored_tables_kernel(const Q *__restrict__ queries, unsigned k, uint32_t *__restrict__ tabs) {
    const Q q = queries[blockIdx.x];
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int d = 2 * (int)threadIdx.x + e - 64;
        if (d >= 0 && d < (int)k) v |= anchored_entry(q, (unsigned)d) << (16 * e);
    }
    tabs[(size_t)blockIdx.x * (kAnchorEntry / 4) + threadIdx.x] = v;
}

// four bases' (A, C) and (G, T) bytes -> their 16-bit one-hots in order
__device__ __forceinline__ int anchored_pair_lo(uint32_t ac, uint32_t gt) { return (int)__builtin_amdgcn_perm(gt, ac, 0x05010400u); } // bases 0, 1
__device__ __forceinline__ int anchored_pair_hi(uint32_t ac, uint32_t gt) { return (int)__builtin_amdgcn_perm(gt, ac, 0x07030602u); } // bases 2, 3
__device__ __forceinline__ i32x8 anchored_operand(uint32_t ac0, uint32_t gt0, uint32_t ac1, uint32_t gt1) {
    return i32x8{anchored_pair_lo(ac0, gt0), anchored_pair_hi(ac0, gt0), anchored_pair_lo(ac1, gt1), anchored_pair_hi(ac1, gt1), 0, 0, 0, 0};
}

// the piece of `len` <= 8 span bytes at a (any alignment) as an operand; bytes behind len read as 'A'.  Only aligned dwords that hold a byte of the piece
// are loaded.  Returns the validity residue of the piece's bytes.
__device__ __forceinline__ uint32_t anchored_piece_ascii(const uint8_t *a, unsigned len, i32x8 &B) {
    const uintptr_t ai = reinterpret_cast<uintptr_t>(a);
    const unsigned sh = (unsigned)(ai & 3u), end = sh + len;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ai - sh);
    uint32_t d0 = 0x41414141u, d1 = 0x41414141u, d2 = 0x41414141u;
    if (len) d0 = p[0];
    if (end > 4) d1 = p[1];
    if (end > 8) d2 = p[2];
    uint32_t x0 = __builtin_amdgcn_alignbyte(d1, d0, sh), x1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const unsigned l1 = len > 4 ? len - 4 : 0;
    const uint32_t keep0 = len >= 4 ? ~0u : (1u << (8 * len)) - 1u, keep1 = l1 >= 4 ? ~0u : (1u << (8 * l1)) - 1u;
    x0 = (x0 & keep0) | (0x41414141u & ~keep0);
    x1 = (x1 & keep1) | (0x41414141u & ~keep1);
    const i32x8 e = onehot8(x0, x1);
    B = anchored_operand((uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]);
    return dword_residue(x0) | dword_residue(x1);
}

__device__ __forceinline__ uint32_t anchored_spread(uint32_t c8) { return (c8 | (c8 << 6) | (c8 << 12) | (c8 << 18)) & 0x03030303u; } // base t -> byte t

// the piece of `len` <= 8 bases from base b of a packed read (b + len <= read_len: the second word is read only where the piece runs into it)
__device__ __forceinline__ void anchored_piece_packed(const uint64_t *__restrict__ words, unsigned b, unsigned len, i32x8 &B) {
    uint32_t c16 = 0;
    if (len) {
        const unsigned sh = 2u * (b & 31u);
        unsigned long long x = words[b >> 5] >> sh;
        if ((b & 31u) + len > 32u) x |= words[(b >> 5) + 1] << (64u - sh);
        c16 = (uint32_t)x & ((1u << (2 * len)) - 1u);
    }
    const uint32_t s0 = anchored_spread(c16 & 0xFFu), s1 = anchored_spread((c16 >> 8) & 0xFFu);
    B = anchored_operand(lut_ac(s0), lut_gt(s0), lut_ac(s1), lut_gt(s1));
}

__device__ __forceinline__ uint32_t anchored_bits(float x) { return __float_as_uint(x); } // (on a copy: pack_distances' note)

// a tile-local pattern -> dist << 26 (ragged: 25) | tilebase + local; all-ones (and every row that starts at 63 / 127) -> a dist field above 32 = none
template <class F> __device__ __forceinline__ uint32_t anchored_global(uint32_t u, uint32_t tilebase) { return ((u << 9) & F::kKeyMask) | (tilebase + (u & 63u)); }

// (b1, b2) <- the two smallest of (b1, b2, g1, g2); b1 <= b2 and g1 <= g2 are keys of distinct queries
__device__ __forceinline__ void anchored_merge(uint32_t &b1, uint32_t &b2, uint32_t g1, uint32_t g2) {
    const uint32_t hi = max(b1, g1), lo2 = min(b2, g2);
    b1 = min(b1, g1);
    b2 = min(hi, lo2);
}

// lanes l and l ^ 32: both copies of x
__device__ __forceinline__ void anchored_halves(uint32_t x, uint32_t &low, uint32_t &high) {
    const auto s = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    low = s[0];
    high = s[1];
}

// P <= 16 rows per query: 16 / P queries in the lane's registers
template <int P, class F>
__device__ __forceinline__ void anchored_reduce(const f32x16 &acc, uint32_t tilebase, uint32_t &b1, uint32_t &b2) {
    uint32_t m1 = ~0u, m2 = ~0u;
#pragma unroll
    for (int i = 0; i < 16 / P; ++i) {
        const float f0 = acc[i * P];
        uint32_t m = anchored_bits(f0);
#pragma unroll
        for (int e = 1; e < P; ++e) {
            const float f = acc[i * P + e];
            m = min(m, anchored_bits(f));
        }
        m2 = min(m2, max(m1, m));
        m1 = min(m1, m);
    }
    anchored_merge(b1, b2, anchored_global<F>(m1, tilebase), anchored_global<F>(m2, tilebase));
}

__device__ __forceinline__ uint32_t anchored_min16(const f32x16 &acc) {
    const float f0 = acc[0];
    uint32_t m = anchored_bits(f0);
#pragma unroll
    for (int e = 1; e < 16; ++e) {
        const float f = acc[e];
        m = min(m, anchored_bits(f));
    }
    return m;
}

// where the lane's accumulators of tile T start: register r is slot 16 h + r, global row 32 T + slot; `offsets`: the admissible offsets of the lane's
// column (the fixed layout's g.offsets, the ragged layout's n_r of the lane's read: admissibility is per (row, column), and a lane holds one column)
template <class F, class G>
__device__ __forceinline__ f32x16 anchored_start(unsigned T, unsigned hh, const G &g, unsigned nq, unsigned offsets) {
    f32x16 c;
    const unsigned pm = (1u << g.lg) - 1u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned row = 32u * T + 16u * hh + (unsigned)r;
        const unsigned s = row & pm, local = row & (g.lg == 6 ? 63u : 31u);
        bool valid;
        if constexpr (G::kRagged) valid = (row >> g.lg) < nq && s < offsets;
        else valid = (row >> g.lg) < nq && s < g.offsets; // (offsets == g.offsets: spelled as before the ragged layout, the generated code is the same)
        c[r] = __uint_as_float(kAnchorBias | ((valid ? g.k : F::kNone) << F::kShift) | local);
    }
    return c;
}

// first: the offset of row 0 (the fixed layout's pos_lo, the ragged layout's a_r)
template <class F>
__device__ __forceinline__ void anchored_store(uint32_t key, unsigned lg, unsigned first, unsigned long long r, uint32_t *__restrict__ query,
                                               uint32_t *__restrict__ pos, uint8_t *__restrict__ dist) {
    const uint32_t d = key >> F::kKeyShift, row = key & ~F::kKeyMask;
    const bool none = d > 32u;
    query[r] = none ? 0xFFFFFFFFu : row >> lg;
    pos[r] = none ? 0xFFFFFFFFu : first + (row & ((1u << lg) - 1u));
    dist[r] = none ? (uint8_t)0xFF : (uint8_t)d;
}

// a lane's read in the ragged layout: base = where the read starts in data (byte, or word when packed), a = its first span base, n = its admissible
// offsets (0 .. g.offsets).  room = last_r - pos_lo: START admits i = pos_lo .. pos_lo + min(room, offsets - 1), END admits e = pos_lo .. the same, that
// is i = room - min(room, offsets - 1) .. room.  Two coalesced 8-byte loads per lane (three when packed); reads are below 2^32 - 1 bases.  The entries are
// loaded one block ahead (AnchorEntries: only the loads, no use), so that the dependent chain table -> span bytes does not start at the top of a block.
struct AnchorLane { unsigned long long base; unsigned a, n; };
struct AnchorEntries { unsigned long long o0, o1, w; };
template <bool PACKED>
__device__ __forceinline__ AnchorEntries anchored_entries(const AnchorBatchGeom &g, unsigned long long r) {
    return AnchorEntries{g.tab[r], g.tab[r + 1], PACKED ? g.wtab[r] : 0ull};
}
template <bool PACKED>
__device__ __forceinline__ AnchorLane anchored_lane(const AnchorBatchGeom &g, const AnchorEntries &e) {
    const long long room = (long long)(e.o1 - e.o0) - (long long)g.k - (long long)g.pos_lo;
    AnchorLane L{PACKED ? e.w : e.o0, g.pos_lo, 0u};
    if (room >= 0) {
        const unsigned more = room < (long long)(g.offsets - 1u) ? (unsigned)room : g.offsets - 1u;
        L.n = more + 1u;
        if (g.end) L.a = (unsigned)(room - (long long)more);
    }
    return L;
}

// data: the reads (ASCII bytes at any alignment, or 8-byte aligned packed words); count >= 1, 1 <= k <= 32, nq >= 1, 1 <= offsets, span = offsets + k - 1
// <= 64.  sq == nullptr: the best triple only.  A bounded grid; a wave walks blocks of 64 reads.  G: the layout policy (AnchorGeom: a fixed stride, one
// range for all reads; AnchorBatchGeom: tables, a range per read); everything that differs is under `if constexpr`, the tile loop has no branch on it.
template <bool PACKED, class G>
__global__ void __launch_bounds__(kAnchorBlock)
reads_anchored_kernel(const uint8_t *__restrict__ data, unsigned long long count, const G g, const uint8_t *__restrict__ tabs, uint32_t *__restrict__ bq,
                      uint32_t *__restrict__ bp, uint8_t *__restrict__ bd, uint32_t *__restrict__ sq, uint32_t *__restrict__ sp, uint8_t *__restrict__ sd,
                      unsigned long long *__restrict__ slot) {
    const unsigned lane = threadIdx.x & 63, n = lane & 31u, hh = lane >> 5;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (kAnchorBlock / 64) + wave_in_block();
    const unsigned long long nwaves = (unsigned long long)gridDim.x * (kAnchorBlock / 64);
    const unsigned long long nblocks = (count + 63) >> 6;
    const unsigned nsteps = (g.span + 15u) >> 4; // wave-uniform
    const unsigned slot_row = 16u * ((n >> 2) & 1u) + (n & 3u) + 4u * (n >> 3); // the slot of A's row n
    using F = AnchorField<G::kRagged>;
    f32x16 c_full[G::kRagged ? kAnchorGroups : 1]; // a tile whose queries all exist, P <= 32: the same for every tile (ragged: per group, set per block)
    if constexpr (!G::kRagged) c_full[0] = anchored_start<F>(0u, hh, g, ~0u, g.offsets);
    // the lane's read of block blk and group gi, clamped at the batch's end: in bounds, never stored
    const auto clamped = [&](unsigned long long blk, int gi) {
        const unsigned long long r = (blk << 6) + 32u * gi + n;
        return r < count ? r : count - 1;
    };
    AnchorEntries ahead[G::kRagged ? kAnchorGroups : 1]; // ragged: the table entries of the wave's next block
    if constexpr (G::kRagged) {
        if (wave < nblocks) {
#pragma unroll
            for (int gi = 0; gi < kAnchorGroups; ++gi) ahead[gi] = anchored_entries<PACKED>(g, clamped(wave, gi));
        }
    }

    for (unsigned long long blk = wave; blk < nblocks; blk += nwaves) {
        i32x8 B[kAnchorGroups][4];
        unsigned first[kAnchorGroups], admit[kAnchorGroups]; // row 0's offset and the admissible offsets of the lane's read
#pragma unroll
        for (int gi = 0; gi < kAnchorGroups; ++gi) {
            const unsigned long long rc = clamped(blk, gi);
            unsigned long long base; // of the read in data: bytes, or words when packed
            unsigned span;           // the span bytes of THIS read: nothing behind them is loaded or validated
            if constexpr (G::kRagged) {
                const AnchorLane L = anchored_lane<PACKED>(g, ahead[gi]);
                base = L.base, first[gi] = L.a, admit[gi] = L.n;
                span = L.n ? L.n + g.k - 1u : 0u;
                c_full[gi] = anchored_start<F>(0u, hh, g, ~0u, L.n);
            } else {
                base = rc * g.stride, first[gi] = g.pos_lo, admit[gi] = g.offsets;
                span = g.span;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned o = 16u * j + 8u * hh;
                const unsigned len = o < span ? (span - o < 8u ? span - o : 8u) : 0u;
                if constexpr (PACKED) {
                    anchored_piece_packed(reinterpret_cast<const uint64_t *>(data) + base, first[gi] + o, len, B[gi][j]);
                } else {
                    const unsigned long long at = base + first[gi] + o;
                    if (__builtin_expect(trip_invalid(anchored_piece_ascii(data + at, len, B[gi][j])), 0)) rescan_bytes(data, at, len, slot);
                }
            }
        }
        if constexpr (G::kRagged) {
            if (blk + nwaves < nblocks) { // behind this block's loads: the next block's entries
#pragma unroll
                for (int gi = 0; gi < kAnchorGroups; ++gi) ahead[gi] = anchored_entries<PACKED>(g, clamped(blk + nwaves, gi));
            }
        }
        uint32_t b1[kAnchorGroups], b2[kAnchorGroups], carry[kAnchorGroups];
#pragma unroll
        for (int gi = 0; gi < kAnchorGroups; ++gi) b1[gi] = b2[gi] = carry[gi] = ~0u;

#pragma unroll 1
        for (unsigned T = 0; T < g.ntiles; ++T) {
            const unsigned row = 32u * T + slot_row, q = row >> g.lg, s = row & ((1u << g.lg) - 1u);
            const bool valid = q < g.nq && s < g.offsets;
            // an invalid row reads the zeros in front of query 0's entry
            const uint8_t *ap = tabs + (valid ? (size_t)q * kAnchorEntry + 2u * (64u + 8u * hh - s) : (size_t)0);
            i32x8 A[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                A[j] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
                if ((unsigned)j < nsteps) {
                    const u32x4 t = *reinterpret_cast<const u32x4_u *>(ap + 32 * j);
                    A[j][0] = (int)t.x, A[j][1] = (int)t.y, A[j][2] = (int)t.z, A[j][3] = (int)t.w;
                }
            }
            const bool full = g.lg <= 5u && ((32u * T + 31u) >> g.lg) < g.nq; // wave-uniform
            f32x16 c, cg[G::kRagged ? kAnchorGroups : 1];
            if constexpr (!G::kRagged) {
                c = full ? c_full[0] : anchored_start<F>(T, hh, g, g.nq, g.offsets);
            } else if (full) { // ONE wave-uniform region for both groups: the partial tile's arithmetic stays out of the full tiles' path
#pragma unroll
                for (int gi = 0; gi < kAnchorGroups; ++gi) cg[gi] = c_full[gi];
            } else {
#pragma unroll
                for (int gi = 0; gi < kAnchorGroups; ++gi) cg[gi] = anchored_start<F>(T, hh, g, g.nq, admit[gi]);
            }
            const uint32_t tilebase = g.lg == 6u ? 32u * (T & ~1u) : 32u * T;
#pragma unroll
            for (int gi = 0; gi < kAnchorGroups; ++gi) {
                if constexpr (G::kRagged) c = cg[gi];
                f32x16 acc = c;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned)j < nsteps) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A[j], B[gi][j], acc, 4, 4, 0, F::kScale, 0, 127);
                switch (g.lg) { // wave-uniform
                case 0: anchored_reduce<1, F>(acc, tilebase, b1[gi], b2[gi]); break;
                case 1: anchored_reduce<2, F>(acc, tilebase, b1[gi], b2[gi]); break;
                case 2: anchored_reduce<4, F>(acc, tilebase, b1[gi], b2[gi]); break;
                case 3: anchored_reduce<8, F>(acc, tilebase, b1[gi], b2[gi]); break;
                case 4: anchored_reduce<16, F>(acc, tilebase, b1[gi], b2[gi]); break;
                default: {
                    uint32_t m = anchored_min16(acc);
                    if (g.lg == 6u) {
                        m = min(m, carry[gi]);
                        carry[gi] = (T & 1u) ? ~0u : m;
                        if (!(T & 1u)) break; // the query's second tile follows
                    }
                    uint32_t lo, hi;
                    anchored_halves(m, lo, hi);
                    const uint32_t key = anchored_global<F>(min(lo, hi), tilebase);
                    b2[gi] = min(b2[gi], max(b1[gi], key));
                    b1[gi] = min(b1[gi], key);
                }
                }
            }
        }

#pragma unroll
        for (int gi = 0; gi < kAnchorGroups; ++gi) {
            if (g.lg <= 4u) { // the two lanes of a read hold different queries
                uint32_t lo1, hi1, lo2, hi2;
                anchored_halves(b1[gi], lo1, hi1);
                anchored_halves(b2[gi], lo2, hi2);
                anchored_merge(b1[gi], b2[gi], hh ? lo1 : hi1, hh ? lo2 : hi2);
            }
            const unsigned long long r = (blk << 6) + 32u * gi + n;
            if (hh == 0u && r < count) {
                anchored_store<F>(b1[gi], g.lg, first[gi], r, bq, bp, bd);
                if (sq) anchored_store<F>(b2[gi], g.lg, first[gi], r, sq, sp, sd);
            }
        }
    }
}

} // namespace bitnuc_dev
