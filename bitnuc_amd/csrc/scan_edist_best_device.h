// scan_edist_best_device.h -- the INDEL-TOLERANT best match and runner-up per read over the WHOLE read (bitnuc_reads_edist_best*, _best_batch* and their
// pattern twins): for every read the smallest (edit distance, query, end) over Q queries, where the edit distance of a query is the Levenshtein distance
// to the best substring of the read (it starts and ends anywhere in the read), and the smallest over the queries other than the winner's.
//
// The kernel of scan_edist_device.h with the span's bound of 64 bases lifted: the same vector-ALU step (edist_step_device.h's: Eq from two levels of selects, the
// 32-bit add as the carry chain, one v_lshl_add + v_min for the running key; kEdistInterleave queries side by side, remainders in groups of 2 and 1), ONE
// READ PER LANE, the lane writes its read's six outputs itself.  What is new: a lane walks its read in PIECES of 64 bases -- the four code registers of the
// anchored form -- and the column state of the interleaved queries (Pv, Mv, score, running key: EdistKeyCols) is carried from piece to piece instead of
// starting fresh.  For each group of queries the lane walks its whole read again (the read is re-read per group: 64 bytes or two words per 64 x U steps);
// ASCII bytes are validated in the first group's walk only.  The next piece's loads are issued ahead of the current piece's 64 steps and held raw (17
// dwords, or two words), aligned and encoded when their turn comes.
// The running key inside the step is (score << 26) + j, j the base index in the read: score <= k <= 32 and j < 2^26 (kEdistBestMaxRead, the host's check)
// keep it in 32 bits.  The top-2 over queries merges (dist << 42 | query << 26 | j) once per query outside the step: queries arrive in ascending order and
// the keys are distinct per query, so the running (best, second) is a 64-bit min / max.
// ASCII: edist_span_ascii's scheme per piece (the aligned dwords that hold a byte of the piece and no other, v_alignbyte, bytes behind the read replaced by
// 'A' for validation only, dword_residue, enc4); packed: piece p of a read is its words 2p and 2p + 1 -- a read starts at a word, so there is no funnel
// shift --, a word that holds no base of the read is never loaded, and the bits above the last base are never stepped over (fixed layout, equal waves) or
// stepped over with Eq forced to 0 (below).
//
// Two layouts, one kernel.  Fixed (EdistBestGeom): reads at a stride, all of g.len bases; the loop runs exactly g.len steps for every lane, nothing is
// masked.  RAGGED (AnchorBatchGeom with pos_lo = 0, START, offsets = 2^32 - 1: the whole read is the window): the lane derives its read from the table
// entries loaded one trip ahead (anchored_entries, anchored_lane); the loop is wave-uniform over the longest read of the wave (edist_wave_max<27>), Eq is 0
// at the steps behind a lane's own length -- the MASKED form of scan_edist_device.h, whose monotonicity argument holds for any length: a column that
// matches nowhere cannot lower D[k][j], and the running minimum keeps the first end.  A wave of equal lengths branches to the unmasked loop.  A lane whose
// read is shorter than k loads nothing, runs masked steps on nothing and writes the fill.
// No LDS, no atomics but the invalid-byte latch, no scratch, 256-lane blocks, a grid bounded at kEdistBlocksPerCu per CU and walked at its stride.
#pragma once
#include "scan_edist_device.h"

namespace bitnuc_dev {

constexpr unsigned kEdistBestEndBits = 26;                      // the end field of the running key: reads of at most 2^26 bases
constexpr unsigned long long kEdistBestMaxRead = 1ull << kEdistBestEndBits;

// stride: bytes (ASCII) or words (packed) per read; len: the bases of every read, k <= len <= 2^26
struct EdistBestGeom { unsigned long long stride; unsigned len, k, nq; static constexpr bool kRagged = false; };

// the columns of U queries with each query's running key: (score << kEdistBestEndBits) + (the base's index), the smallest score and its first end
template <int U> struct EdistKeyCols : EdistCols<U> { uint32_t key[U]; };

// a piece's raw loads, held across the previous piece's steps
struct EdistPieceAscii { uint32_t d[17]; };
struct EdistPiecePacked { unsigned long long w0, w1; };

// the aligned dwords that hold one of the n <= 64 bytes at a (n == 0: none); every other register reads as 'A's
__device__ __forceinline__ void edist_piece_load(const uint8_t *a, unsigned n, EdistPieceAscii &pc) {
    const uintptr_t ai = reinterpret_cast<uintptr_t>(a);
    const unsigned sh = (unsigned)(ai & 3u), end = n ? sh + n : 0u;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ai - sh);
#pragma unroll
    for (unsigned i = 0; i < 17; ++i) {
        pc.d[i] = 0x41414141u;
        if (4u * i < end) pc.d[i] = p[i]; // holds a byte of the piece
    }
}

// ... as 2-bit codes, 16 per register; returns the validity residue of the piece's n bytes (edist_span_ascii's second half)
__device__ __forceinline__ uint32_t edist_piece_codes(const EdistPieceAscii &pc, unsigned sh, unsigned n, uint32_t (&span)[4]) {
    uint32_t bad = 0;
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        uint32_t codes = 0;
#pragma unroll
        for (unsigned e = 0; e < 4; ++e) {
            const unsigned i = 4u * w + e;
            const unsigned len = n > 4u * i ? (n - 4u * i < 4u ? n - 4u * i : 4u) : 0u; // the piece's bytes in this dword
            uint32_t x = __builtin_amdgcn_alignbyte(pc.d[i + 1], pc.d[i], sh);
            const uint32_t keep = len >= 4u ? ~0u : (1u << (8u * len)) - 1u;
            x = (x & keep) | (0x41414141u & ~keep);
            bad |= dword_residue(x);
            uint32_t unused = 0;
            codes |= enc4(x, unused) << (8u * e);
        }
        span[w] = codes;
    }
    return bad;
}

// words 2p and 2p + 1 of a read of len bases: only those that hold a base of it
__device__ __forceinline__ void edist_piece_load(const uint64_t *__restrict__ words, unsigned p, unsigned len, EdistPiecePacked &pc) {
    pc.w0 = 0, pc.w1 = 0;
    if (len > 64u * p) pc.w0 = words[2ull * p];
    if (len > 64u * p + 32u) pc.w1 = words[2ull * p + 1ull];
}

// cnt <= 64 steps (wave-uniform) over a piece whose first base is base j0 of the read: the anchored kernel's loop (edist_eq, edist_step) with the state in c.  MASKED: Eq is 0 at the
// steps at and behind base `len` of the lane's read
template <int U, bool MASKED>
__device__ __forceinline__ void edist_best_steps(const uint32_t (&span)[4], unsigned cnt, unsigned j0, unsigned top, EdistKeyCols<U> &c, unsigned len) {
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        if (16u * w >= cnt) break; // wave-uniform
        uint32_t codes = span[w];
        const unsigned n16 = cnt - 16u * w < 16u ? cnt - 16u * w : 16u;
#pragma unroll 1
        for (unsigned s = 0; s < n16; ++s) {
            const uint32_t lo = 0u - (codes & 1u); // the base's low code bit as a mask
            const bool hi = (codes & 2u) != 0u;
            codes >>= 2;
            const unsigned j = j0 + 16u * w + s; // the step's end is j + 1
            uint32_t live = ~0u;
            if constexpr (MASKED) live = j < len ? ~0u : 0u; // once per step, not per query
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t eq = edist_eq(c, u, lo, hi);
                if constexpr (MASKED) eq &= live;
                edist_step(c, u, eq, top, [&](uint32_t sc) { c.key[u] = min(c.key[u], (sc << kEdistBestEndBits) + j); });
            }
        }
    }
}

// Queries q0 .. q0 + U - 1 against the lane's whole read, piece by piece: every query's (dist, first end) merged into the running (best, second) keys.
// data + base: the read's first byte (ASCII; base is also its index for the latch) or word (packed); len: the lane's bases (0: nothing is loaded); nmax: the
// steps, wave-uniform, >= len.  Invalid bytes are latched where q0 == 0 only.
template <int U, bool MASKED, bool PACKED>
__device__ __forceinline__ void edist_best_queries(const uint8_t *__restrict__ data, unsigned long long base, unsigned len, unsigned nmax, unsigned k,
                                                   const u32x4 *__restrict__ tabs, unsigned q0, unsigned long long &b1, unsigned long long &b2,
                                                   unsigned long long *__restrict__ slot) {
    EdistKeyCols<U> c;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        edist_cols_init(c, u, tabs[q0 + u], k);
        c.key[u] = ~0u;
    }
    const unsigned top = k - 1u;
    const auto bases_of = [len](unsigned p) { return len > 64u * p ? (len - 64u * p < 64u ? len - 64u * p : 64u) : 0u; }; // the lane's bases in piece p
    if constexpr (PACKED) {
        const uint64_t *words = reinterpret_cast<const uint64_t *>(data) + base;
        EdistPiecePacked cur, nxt;
        edist_piece_load(words, 0u, len, cur);
#pragma unroll 1
        for (unsigned p = 0; 64u * p < nmax; ++p) {
            edist_piece_load(words, p + 1u, len, nxt); // ahead of this piece's steps (nothing behind the read)
            const uint32_t span[4] = {(uint32_t)cur.w0, (uint32_t)(cur.w0 >> 32), (uint32_t)cur.w1, (uint32_t)(cur.w1 >> 32)};
            const unsigned cnt = nmax - 64u * p < 64u ? nmax - 64u * p : 64u;
            edist_best_steps<U, MASKED>(span, cnt, 64u * p, top, c, len);
            cur = nxt;
        }
    } else {
        const uint8_t *a = data + base;
        const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(a) & 3u); // of every piece: they are 64 bytes apart
        EdistPieceAscii cur, nxt;
        edist_piece_load(a, bases_of(0u), cur);
#pragma unroll 1
        for (unsigned p = 0; 64u * p < nmax; ++p) {
            edist_piece_load(a + 64ull * (p + 1u), bases_of(p + 1u), nxt); // ahead of this piece's steps (nothing behind the read)
            uint32_t span[4];
            const unsigned n = bases_of(p);
            const uint32_t bad = edist_piece_codes(cur, sh, n, span);
            if (q0 == 0u && __builtin_expect(trip_invalid(bad), 0)) rescan_bytes(data, base + 64ull * p, n, slot);
            const unsigned cnt = nmax - 64u * p < 64u ? nmax - 64u * p : 64u;
            edist_best_steps<U, MASKED>(span, cnt, 64u * p, top, c, len);
#pragma unroll
            for (unsigned i = 0; i < 17; ++i) cur.d[i] = nxt.d[i];
        }
    }
    constexpr uint32_t kEndMask = (1u << kEdistBestEndBits) - 1u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long g = ((unsigned long long)(c.key[u] >> kEdistBestEndBits) << 42) | ((unsigned long long)(q0 + (unsigned)u) << kEdistBestEndBits) |
                                     (unsigned long long)(c.key[u] & kEndMask);
        const unsigned long long hi = b1 > g ? b1 : g;
        b2 = b2 < hi ? b2 : hi;
        b1 = b1 < g ? b1 : g;
    }
}

// every query against the lane's read: groups of kEdistInterleave, then of 2 and 1
template <bool MASKED, bool PACKED>
__device__ __forceinline__ void edist_best_all_queries(const uint8_t *__restrict__ data, unsigned long long base, unsigned len, unsigned nmax, unsigned k, unsigned nq,
                                                       const u32x4 *__restrict__ tabs, unsigned long long &b1, unsigned long long &b2,
                                                       unsigned long long *__restrict__ slot) {
    edist_query_groups(nq, [&](auto U, unsigned q0) { edist_best_queries<decltype(U)::value, MASKED, PACKED>(data, base, len, nmax, k, tabs, q0, b1, b2, slot); });
}

// a key -> the read's triple; all-ones (no query but the winner, no window): the fill
__device__ __forceinline__ void edist_best_store(unsigned long long key, unsigned long long r, uint32_t *__restrict__ query, uint32_t *__restrict__ end,
                                                 uint8_t *__restrict__ dist) {
    const bool none = key == ~0ull;
    query[r] = none ? 0xFFFFFFFFu : (uint32_t)(key >> kEdistBestEndBits) & 0xFFFFu;
    end[r] = none ? 0xFFFFFFFFu : ((uint32_t)key & ((1u << kEdistBestEndBits) - 1u)) + 1u;
    dist[r] = none ? (uint8_t)0xFF : (uint8_t)(key >> 42);
}

// data: the reads (ASCII bytes at any alignment, or 8-byte aligned packed words); count >= 1, 1 <= k <= 32, 1 <= nq <= 65536; tabs: nq entries of
// edist_tables_kernel; reads of at most 2^26 bases; fixed: k <= g.len.  sq == nullptr: the best triple only.  A bounded grid; a lane walks reads at the
// grid's stride.  G: the layout policy (EdistBestGeom: a fixed stride and length; AnchorBatchGeom: tables, the whole read as the window).
template <bool PACKED, class G>
__global__ void __launch_bounds__(kEdistBlock)
reads_edist_best_kernel(const uint8_t *__restrict__ data, unsigned long long count, const G g, const u32x4 *__restrict__ tabs, uint32_t *__restrict__ bq,
                        uint32_t *__restrict__ be, uint8_t *__restrict__ bd, uint32_t *__restrict__ sq, uint32_t *__restrict__ se, uint8_t *__restrict__ sd,
                        unsigned long long *__restrict__ slot) {
    const unsigned long long step = (unsigned long long)gridDim.x * kEdistBlock;
    unsigned long long r = (unsigned long long)blockIdx.x * kEdistBlock + threadIdx.x;
    if constexpr (!G::kRagged) {
        for (; r < count; r += step) {
            unsigned long long b1 = ~0ull, b2 = ~0ull;
            edist_best_all_queries<false, PACKED>(data, r * g.stride, g.len, g.len, g.k, g.nq, tabs, b1, b2, slot);
            edist_best_store(b1, r, bq, be, bd);
            if (sq) edist_best_store(b2, r, sq, se, sd);
        }
    } else {
        AnchorEntries ahead{0, 0, 0}; // the table entries of the lane's next read
        if (r < count) ahead = anchored_entries<PACKED>(g, r);
        for (; r < count; r += step) {
            const AnchorLane L = anchored_lane<PACKED>(g, ahead);
            const unsigned len = L.n ? L.n + g.k - 1u : 0u; // the read's bases; 0 where it is shorter than k: nothing of it is loaded or validated
            if (r + step < count) ahead = anchored_entries<PACKED>(g, r + step);
            const unsigned nmax = edist_wave_max<kEdistBestEndBits + 1>(len); // wave-uniform; 0: no lane of the wave has a window
            unsigned long long b1 = ~0ull, b2 = ~0ull;
            if (__builtin_amdgcn_ballot_w64(len != nmax) == 0ull) { // a wave of equal lengths: the fixed layout's loop
                if (nmax) edist_best_all_queries<false, PACKED>(data, L.base, len, nmax, g.k, g.nq, tabs, b1, b2, slot);
            } else {
                edist_best_all_queries<true, PACKED>(data, L.base, len, nmax, g.k, g.nq, tabs, b1, b2, slot);
                if (!len) b1 = b2 = ~0ull; // the masked steps of a lane without a window made keys of no window
            }
            edist_best_store(b1, r, bq, be, bd);
            if (sq) edist_best_store(b2, r, sq, se, sd);
        }
    }
}

} // namespace bitnuc_dev
