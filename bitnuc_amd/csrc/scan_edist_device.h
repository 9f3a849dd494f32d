// scan_edist_device.h -- the INDEL-TOLERANT anchored best match and runner-up per read (bitnuc_reads_edist_anchored*, bitnuc_reads_pattern_edist_anchored*):
// for every read of a fixed-length batch the smallest (edit distance, query, end) over Q queries, where the edit distance of a query is the Levenshtein
// distance to the best substring of the read's span [pos_lo, hi_eff + k) (the substring starts and ends anywhere in the span), and the smallest over the
// queries other than the winner's.
//
// A column's start from its table entry, Eq and THE STEP are edist_step_device.h's (the edist_col_* forms: this kernel keeps its columns in arrays of its
// own), as are the query groups and the wave maximum; the three other kernels of the family share them.
// A vector-ALU kernel, not a matrix-core product: the bit-parallel recurrence (Myers 1999 in Hyyro's form) carries a 32-bit add through the column of one
// (read, query) pair at every span base; it is a carry chain, not a contraction.  k <= 32 keeps a column's vertical deltas in two 32-bit registers (Pv,
// Mv), the span's n <= 64 bases are four registers of 2-bit codes per lane, a query's score and running key are two more.  No LDS, no spill, no atomics but the
// invalid-byte latch, no finish kernel, no per-read scratch: ONE READ PER LANE, and the lane writes its read's six outputs itself.
//   per span base t_j:   Eq = Peq[t_j]                      (bit i set <=> query position i matches t_j)
//                        Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
//                        Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
//                        score += bit k-1 of Ph, -= bit k-1 of Mh          (D[k][j]; starts at k = D[k][0])
//                        Ph <<= 1;  Mh <<= 1                  (no carry-in: D[0][j] = 0, the substring starts anywhere)
//                        Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
// Bits at and above k of every word are junk that never travels down (the add carries upwards, the shifts go left), so only Peq is masked to k bits and
// only bit k - 1 is tested: k = 32 needs no 1u << 32 anywhere.  The running minimum is one v_min of (score << 6 | j - 1): the smallest score and its
// first end.  20 vector instructions per (read, query, span base) in the loop of four queries (DESIGN.md 3.4 has the count by opcode and what was tried).
// Queries: a 16-byte entry per query in context scratch, Peq[A, C, G, T] masked to k bits, built in-stream by edist_tables_kernel from a 2-bit query or
// copied from a pattern's allow[] (the sets ARE the match masks: patterns cost nothing in the main kernel, which has one form for both kinds).  The query
// loop is wave-uniform; a lane runs kEdistInterleave queries side by side through one walk over its span, so the extraction of a base's two code bits
// and the loop's scalar bookkeeping are paid once per kEdistInterleave columns; remainders of Q run as groups of 2 and 1.  Eq is two levels of
// selects on the base's two code bits (two three-input bit ops and a v_cndmask), not a lookup.
// Top-2: queries arrive in ascending order and a query's key is (dist << 22 | query << 6 | end - pos_lo - 1), distinct per query, so the running
// (best, second) is min / max only.
// ASCII: the lane loads the aligned dwords that hold a byte of its span (nothing outside such a dword is touched), aligns them (v_alignbyte), replaces the
// bytes behind the span by 'A', validates with dword_residue (the first invalid span byte of the batch is latched by atomicMin) and packs four codes per
// dword (enc4).  Packed: the one to three words that hold the span and a funnel shift; bits behind the span are never looked at.
//
// Two layouts, one kernel (the template parameter G, everything that differs under `if constexpr`), as reads_anchored_kernel has them.  Fixed (EdistGeom):
// reads at a stride, one span for all of them -- the text above.  RAGGED (AnchorBatchGeom, bitnuc_reads_edist_anchored_batch*): reads behind an offsets
// table, the range counted from each read's start or from its end.  A lane already is one read, so the layout is per-lane data: the lane loads its read's
// table entries (AnchorEntries, one trip ahead) and derives a_r, its first span base, and n_r, its admissible offsets (anchored_lane); it loads and
// validates its own n_r + k - 1 span bytes only (none when n_r == 0: such a lane writes the fill).  The recurrence loop stays wave-uniform, over the widest
// span among the wave's lanes.  A lane with a shorter span is not disturbed by the steps behind it if their Eq is 0: such a column cannot lower D[k][j]
// (D[i][j + 1] >= D[i][j] for every i when column j + 1 matches nowhere, by induction over i), and the running minimum keeps the first end.  So the
// span sits at steps 0 .. len_r - 1 and Eq is ANDed with a per-step lane mask: one more vector instruction per (query, step), and none in a wave whose
// lanes all have the widest span the arguments allow -- that case branches, wave-uniformly, to the fixed layout's loop.  The key's end field stays
// relative to a_r; the store adds a_r.  The fixed instantiations' instructions are those of the kernel before it had a second layout.
#pragma once
#include "device_prims.h"
#include "edist_step_device.h"    // edist_col_init, edist_col_eq, edist_col_step, edist_query_groups, edist_wave_max
#include "scan_anchored_device.h" // the ragged layout: AnchorBatchGeom, AnchorEntries, anchored_entries, anchored_lane
#include "scan_mfma_device.h"     // PatternSets, pattern_of_2bit, dword_residue, trip_invalid

namespace bitnuc_dev {

constexpr int kEdistBlock = 256;        // four waves, nothing shared between them
constexpr unsigned kEdistBlocksPerCu = 8; // the grid's bound: reads behind it are walked in a grid-stride loop

// stride: bytes (ASCII) or words (packed) per read; n: the span's bases, k <= n <= 64
struct EdistGeom { unsigned long long stride; unsigned pos_lo, n, k, nq; static constexpr bool kRagged = false; };

// the match masks of a query, by its kind (the two QueryKind kinds): an exact query is the pattern of its singletons
__device__ __forceinline__ PatternSets edist_sets(unsigned long long q, unsigned k) { return pattern_of_2bit(q, k); }
__device__ __forceinline__ PatternSets edist_sets(const PatternSets &p, unsigned) { return p; }

// entry q: Peq[c] = the positions < k of query q that base code c matches
template <class Q>
__global__ void __launch_bounds__(64) edist_tables_kernel(const Q *__restrict__ queries, unsigned nq, unsigned k, u32x4 *__restrict__ tabs) {
    const unsigned q = blockIdx.x * 64u + threadIdx.x;
    if (q >= nq) return;
    const PatternSets p = edist_sets(queries[q], k);
    const uint32_t ones = kmer_ones(k);
    tabs[q] = u32x4{p.allow[0] & ones, p.allow[1] & ones, p.allow[2] & ones, p.allow[3] & ones};
}

// the span of `n` bases at a (any alignment) as 2-bit codes, 16 per register; returns the validity residue of the span's bytes
__device__ __forceinline__ uint32_t edist_span_ascii(const uint8_t *a, unsigned n, uint32_t (&span)[4]) {
    const uintptr_t ai = reinterpret_cast<uintptr_t>(a);
    const unsigned sh = (unsigned)(ai & 3u), end = sh + n;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ai - sh);
    uint32_t d[17];
#pragma unroll
    for (unsigned i = 0; i < 17; ++i) {
        d[i] = 0x41414141u;
        if (4u * i < end) d[i] = p[i]; // holds a span byte
    }
    uint32_t bad = 0;
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        uint32_t codes = 0;
#pragma unroll
        for (unsigned e = 0; e < 4; ++e) {
            const unsigned i = 4u * w + e;
            const unsigned len = n > 4u * i ? (n - 4u * i < 4u ? n - 4u * i : 4u) : 0u; // the span's bytes in this dword (wave-uniform in the fixed layout)
            uint32_t x = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
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

// the span of `n` bases from base b of a packed read: only the words that hold a span base are loaded; bits behind the span are junk
__device__ __forceinline__ void edist_span_packed(const uint64_t *__restrict__ words, unsigned b, unsigned n, uint32_t (&span)[4]) {
    const unsigned first = b >> 5, sh = 2u * (b & 31u), last = (b & 31u) + n; // the span ends in word first + (last - 1) / 32
    unsigned long long w0 = words[first], w1 = 0, w2 = 0;
    if (last > 32u) w1 = words[first + 1];
    if (last > 64u) w2 = words[first + 2];
    unsigned long long lo = w0, hi = w1;
    if (sh) { // (a shift by 64 - sh = 64 is no shift C++ has)
        lo = (w0 >> sh) | (w1 << (64u - sh));
        hi = (w1 >> sh) | (w2 << (64u - sh));
    }
    span[0] = (uint32_t)lo, span[1] = (uint32_t)(lo >> 32), span[2] = (uint32_t)hi, span[3] = (uint32_t)(hi >> 32);
}

// queries q0 .. q0 + U - 1 against the lane's span: every query's (dist, first end) merged into the running (best, second) keys.  n: the steps, wave-uniform.
// MASKED (the ragged layout's waves of unequal spans): the lane's span has len <= n bases, Eq is 0 at the steps behind them
template <int U, bool MASKED = false>
__device__ __forceinline__ void edist_queries(const uint32_t (&span)[4], unsigned n, unsigned k, const u32x4 *__restrict__ tabs, unsigned q0, uint32_t &b1,
                                              uint32_t &b2, unsigned len = 0) {
    uint32_t pa[U], pc[U], pg[U], pt[U], pv[U], mv[U], sc[U], key[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        edist_col_init(tabs[q0 + u], k, pa[u], pc[u], pg[u], pt[u], pv[u], mv[u], sc[u]);
        key[u] = ~0u;
    }
    const unsigned top = k - 1u;
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        if (16u * w >= n) break; // wave-uniform
        uint32_t codes = span[w];
        const unsigned cnt = n - 16u * w < 16u ? n - 16u * w : 16u;
#pragma unroll 1
        for (unsigned s = 0; s < cnt; ++s) {
            const uint32_t lo = 0u - (codes & 1u); // the base's low code bit as a mask
            const bool hi = (codes & 2u) != 0u;
            codes >>= 2;
            const unsigned j = 16u * w + s; // the step's end is pos_lo + j + 1
            uint32_t live = ~0u;
            if constexpr (MASKED) live = j < len ? ~0u : 0u; // once per step, not per query
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t eq = edist_col_eq(pa[u], pc[u], pg[u], pt[u], lo, hi);
                if constexpr (MASKED) eq &= live;
                uint32_t &ku = key[u];
                edist_col_step(eq, pv[u], mv[u], sc[u], top, [&ku, j](uint32_t d) { ku = min(ku, (d << 6) + j); });
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t g = ((key[u] >> 6) << 22) | ((q0 + (unsigned)u) << 6) | (key[u] & 63u);
        b2 = min(b2, max(b1, g));
        b1 = min(b1, g);
    }
}

// a key -> the read's triple; all-ones (no query but the winner): the fill.  first: the offset in the read of the span's first base
__device__ __forceinline__ void edist_store(uint32_t key, unsigned first, unsigned long long r, uint32_t *__restrict__ query, uint32_t *__restrict__ end,
                                            uint8_t *__restrict__ dist) {
    const bool none = key == ~0u;
    query[r] = none ? 0xFFFFFFFFu : (key >> 6) & 0xFFFFu;
    end[r] = none ? 0xFFFFFFFFu : first + (key & 63u) + 1u;
    dist[r] = none ? (uint8_t)0xFF : (uint8_t)(key >> 22);
}

// every query against the lane's span (edist_queries' parameters): groups of kEdistInterleave, then of 2 and 1
template <bool MASKED>
__device__ __forceinline__ void edist_all_queries(const uint32_t (&span)[4], unsigned n, unsigned k, unsigned nq, const u32x4 *__restrict__ tabs, uint32_t &b1,
                                                  uint32_t &b2, unsigned len) {
    edist_query_groups(nq, [&](auto U, unsigned q0) { edist_queries<decltype(U)::value, MASKED>(span, n, k, tabs, q0, b1, b2, len); });
}

// data: the reads (ASCII bytes at any alignment, or 8-byte aligned packed words); count >= 1, 1 <= k <= 32, k <= n <= 64, 1 <= nq <= 65536; tabs: nq entries
// of edist_tables_kernel.  sq == nullptr: the best triple only.  A bounded grid; a lane walks reads at the grid's stride.  G: the layout policy (EdistGeom:
// a fixed stride, one span for all reads; AnchorBatchGeom: tables, a span per read, of at most g.span = g.offsets + k - 1 bases; its lg and ntiles are unused).
template <bool PACKED, class G = EdistGeom>
__global__ void __launch_bounds__(kEdistBlock)
reads_edist_kernel(const uint8_t *__restrict__ data, unsigned long long count, const G g, const u32x4 *__restrict__ tabs, uint32_t *__restrict__ bq,
                   uint32_t *__restrict__ be, uint8_t *__restrict__ bd, uint32_t *__restrict__ sq, uint32_t *__restrict__ se, uint8_t *__restrict__ sd,
                   unsigned long long *__restrict__ slot) {
    const unsigned long long step = (unsigned long long)gridDim.x * kEdistBlock;
    if constexpr (!G::kRagged) {
        for (unsigned long long r = (unsigned long long)blockIdx.x * kEdistBlock + threadIdx.x; r < count; r += step) {
            uint32_t span[4];
            if constexpr (PACKED) {
                edist_span_packed(reinterpret_cast<const uint64_t *>(data) + r * g.stride, g.pos_lo, g.n, span);
            } else {
                const unsigned long long at = r * g.stride + g.pos_lo;
                if (__builtin_expect(trip_invalid(edist_span_ascii(data + at, g.n, span)), 0)) rescan_bytes(data, at, g.n, slot);
            }
            uint32_t b1 = ~0u, b2 = ~0u;
            unsigned q = 0; // (spelled here: through edist_all_queries the fixed instantiations compile to other code)
#pragma unroll 1
            for (; q + kEdistInterleave <= g.nq; q += kEdistInterleave) edist_queries<kEdistInterleave>(span, g.n, g.k, tabs, q, b1, b2);
            if (g.nq - q >= 2u) { edist_queries<2>(span, g.n, g.k, tabs, q, b1, b2); q += 2u; }
            if (g.nq - q >= 1u) edist_queries<1>(span, g.n, g.k, tabs, q, b1, b2);
            edist_store(b1, g.pos_lo, r, bq, be, bd);
            if (sq) edist_store(b2, g.pos_lo, r, sq, se, sd);
        }
    } else {
        unsigned long long r = (unsigned long long)blockIdx.x * kEdistBlock + threadIdx.x;
        AnchorEntries ahead{0, 0, 0}; // the table entries of the lane's next read
        if (r < count) ahead = anchored_entries<PACKED>(g, r);
        for (; r < count; r += step) {
            const AnchorLane L = anchored_lane<PACKED>(g, ahead);
            const unsigned len = L.n ? L.n + g.k - 1u : 0u; // the span bases of THIS read: nothing behind them is loaded or validated
            uint32_t span[4] = {0u, 0u, 0u, 0u};
            if (len) {
                if constexpr (PACKED) {
                    edist_span_packed(reinterpret_cast<const uint64_t *>(data) + L.base, L.a, len, span);
                } else {
                    const unsigned long long at = L.base + L.a;
                    if (__builtin_expect(trip_invalid(edist_span_ascii(data + at, len, span)), 0)) rescan_bytes(data, at, len, slot);
                }
            }
            if (r + step < count) ahead = anchored_entries<PACKED>(g, r + step); // behind this read's loads: the next read's entries
            uint32_t b1 = ~0u, b2 = ~0u;
            if (__builtin_amdgcn_ballot_w64(len != g.span) == 0ull) { // every lane has the widest span: the fixed layout's loop
                edist_all_queries<false>(span, g.span, g.k, g.nq, tabs, b1, b2, 0u);
            } else {
                const unsigned widest = edist_wave_max<7>(len); // wave-uniform; 0: no lane of the wave has a window
                if (widest) edist_all_queries<true>(span, widest, g.k, g.nq, tabs, b1, b2, len);
                if (!len) b1 = b2 = ~0u; // the masked steps of a lane without a span made keys of no window
            }
            edist_store(b1, L.a, r, bq, be, bd);
            if (sq) edist_store(b2, L.a, r, sq, se, sd);
        }
    }
}

} // namespace bitnuc_dev

