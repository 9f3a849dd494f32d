// kmer.hip -- k-mer compositions of the hot path behind the C ABI (include/bitnuc_hip.h): batched as_2bit over many
// <= 32-mers (BASELINE config 3, README.md:52-56), every window of a sequence (src/lib.rs:170-173), the sliding pack +
// Hamming scan (config 5: packing/mod.rs:80-110 o hamming/scalar.rs:11-48) and bulk hdist (hamming/multi.rs:121-160).
// Kernels: kmer_device.h; config 5 on the matrix cores: scan_mfma_device.h; the same scan and count on packed words: scan_packed_device.h; the hit
// lists of both: scan_hits_device.h; the count for many queries at once: scan_multi_device.h; the best match per query: scan_best_device.h; the mismatch histogram per query: scan_hist_device.h; the best match per read of a
// fixed-length batch: scan_reads_device.h; ... of a ragged batch: scan_reads_batch_device.h; the indel-tolerant search along a reference: scan_edist_ref_device.h, its hit list: scan_edist_hits_device.h; where an alignment starts: scan_edist_start_device.h; the 3' adapter per read: scan_edist_adapter_device.h.  The launchers, their argument checks and the host forms' chunk loops are here; the host side of the searches
// along a reference -- inputs, searches, the two skeletons -- is ref_dispatch.h, that of every per-read matcher reads_dispatch.h.
#include "runtime.h"

#include <type_traits>

#include "kmer_device.h"
#include "scan_mfma_device.h"
#include "scan_packed_device.h"
#include "scan_hits_device.h"
#include "scan_multi_device.h"
#include "scan_best_device.h"
#include "scan_reads_device.h"
#include "scan_reads_batch_device.h"
#include "scan_anchored_device.h"
#include "scan_edist_device.h"
#include "scan_edist_best_device.h"
#include "scan_edist_ref_device.h"
#include "scan_edist_hits_device.h"
#include "scan_edist_start_device.h"
#include "scan_edist_adapter_device.h"
#include "scan_hist_device.h"
#include "scan_mfma_host.h"
#include "scan_hits_host.h"
#include "scan_multi_host.h"
#include "scan_best_host.h"
#include "reads_best_host.h"
#include "reads_best2_host.h"
#include "reads_anchored_host.h"
#include "reads_anchored_batch_host.h"
#include "reads_edist_host.h"
#include "reads_edist_best_host.h"
#include "kmer_edist_host.h"
#include "edist_start_host.h"
#include "reads_edist_adapter_host.h"
#include "reads_batch_host.h"
#include "scan_hist_host.h"
#include "pattern_host.h"
#include "host_word.h"
#include "host_pipe.h"

using namespace bitnuc_dev;
using namespace bitnuc_rt;
using namespace bitnuc_host;

namespace {
// a host-pointer call's first invalid byte as its error
inline int fail_invalid_base(bitnuc_err *err, uint8_t byte, uint64_t index) {
    if (err) { memset(err, 0, sizeof *err); err->status = BITNUC_INVALID_BASE; err->byte = byte; err->index = index; }
    return BITNUC_INVALID_BASE;
}

// ---- the legs of a k-mer batch: templates the product instantiates with the shipped values (ShippedLegs) and the evidence build with others
template <bool AL, bool NL, bool NS, int U>
hipError_t dense_t(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long items, unsigned long long *o, unsigned long long *slot, int kb) {
    const unsigned grid = grid_for(c, (items + (kb / 64) * U - 1) / ((kb / 64) * U), kb);
    kmer_dense_kernel<AL, NL, NS, U><<<grid, kb, 0, c->stream>>>(kmers, (unsigned)k, items, o, slot);
    return hipGetLastError();
}

template <bool NT, int U>
hipError_t slide2_t(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) {
    const unsigned grid = grid_for(c, (rounds + (unsigned long long)U * (kBlock / 64) - 1) / ((unsigned long long)U * (kBlock / 64)));
    kmer_slide2_kernel<NT, U><<<grid, kBlock, 0, c->stream>>>(kmers, (unsigned)k, rounds, o, slot);
    return hipGetLastError();
}

template <bool NT, int P>
hipError_t slide_t(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) {
    const unsigned grid = grid_for(c, (rounds + (unsigned long long)P * (kBlock / 64) - 1) / ((unsigned long long)P * (kBlock / 64)));
#define SLIDE(S) kmer_slide_kernel<S, NT, P><<<grid, kBlock, 0, c->stream>>>(kmers, (unsigned)k, rounds, o, slot)
    switch (stride) {
    case 1: SLIDE(1); break;
    case 2: SLIDE(2); break;
    case 4: SLIDE(4); break;
    case 8: SLIDE(8); break;
    default: SLIDE(16); break;
    }
#undef SLIDE
    return hipGetLastError();
}

// which legs a batch may use and the kernels they launch: nt loads and stores, one item per wave, 4 rounds per slide2 trip
// (profiles/r03_ab_windows.txt), one round per slide trip
struct ShippedLegs {
    bool dense = true, slide2 = true, slide = true;
    hipError_t launch_dense(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long items, unsigned long long *o, unsigned long long *slot) const {
        if (!aligned16(kmers)) return dense_t<false, false, false, 1>(c, kmers, k, items, o, slot, kKmerBlock);
        return dense_t<true, (kDensePolicy & 1) != 0, (kDensePolicy & 2) != 0, kDenseUnroll>(c, kmers, k, items, o, slot, kKmerBlock);
    }
    hipError_t launch_slide2(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) const {
        return slide2_t<kSlideNt, kSlide2Rounds>(c, kmers, k, rounds, o, slot);
    }
    hipError_t launch_slide(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) const {
        return slide_t<kSlideNt, kSlideRounds>(c, kmers, k, stride, rounds, o, slot);
    }
};

template <class Legs>
hipError_t batch_legs(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, size_t count, unsigned long long *o, unsigned long long *slot, const Legs &L) {
    size_t done = 0;
    hipError_t rc;
    if (stride == k && count >= 64 && L.dense) {
        // dense layout: whole waves of 64 k-mers go through the bulk-encode-shaped kernel
        const unsigned long long items = count / 64;
        if ((rc = L.launch_dense(c, kmers, k, items, o, slot)) != hipSuccess) return rc;
        done = items * 64;
        if (done == count) return hipSuccess;
    }
    if (stride == 1 && done == 0 && L.slide2 && aligned16(kmers) && aligned16(o) && count - 1 + k >= 1056) {
        // every window of a sequence (src/lib.rs:170-173): line-aligned rounds of 1024 windows, computed where they are stored
        const unsigned long long rounds = (count - 1 + k - 32) >> 10; // round r reads bytes [1024 r, 1024 r + 1056)
        if ((rc = L.launch_slide2(c, kmers, k, rounds, o, slot)) != hipSuccess) return rc;
        done = (size_t)(rounds << 10); // < count: the windows of the last partial KiB follow below
    }
    // (k >= stride: every byte of the span belongs to some k-mer, so validating whole 16-byte groups examines no byte the
    // reference's loop would not; with gaps between k-mers the general kernel looks at each k-mer's own bytes only)
    if ((stride == 1 || stride == 2 || stride == 4 || stride == 8 || stride == 16) && k >= stride && done == 0 && L.slide &&
        aligned16(kmers) && aligned16(o) && (count - 1) * stride + k >= 1024) {
        // windows at a small power-of-two stride (1 = every window of a sequence): whole 1 KiB wave rounds through the
        // sliding kernel, 992 / stride windows each; the round that would read past the batch's last byte is left over
        const unsigned long long rounds = ((count - 1) * stride + k - 1024) / kScanWaveWindows + 1;
        if ((rc = L.launch_slide(c, kmers, k, stride, rounds, o, slot)) != hipSuccess) return rc;
        done = (size_t)(rounds * (kScanWaveWindows / stride));
        if (done >= count) return hipSuccess;
    }
    if (stride >= 3 && stride < 32 && k >= stride && done == 0 && L.slide && aligned16(kmers) && (count - 1) * stride + k >= 1024) {
        // any other small stride with overlapping k-mers: the sliding round with per-lane window selection
        const unsigned long long rounds = ((count - 1) * stride + k - 1024) / kScanWaveWindows + 1;
        const unsigned grid = grid_for(c, (rounds + kBlock / 64 - 1) / (kBlock / 64));
        const unsigned magic = (unsigned)((0x100000000ull + stride - 1) / stride); // exact floor(t / stride) for t < 2^16
        const unsigned long long magic64 = ~0ull / stride + 1; // stride >= 3: no overflow
        kmer_slide_any_kernel<<<grid, kBlock, 0, c->stream>>>(kmers, (unsigned)k, (unsigned)stride, magic, magic64, rounds, o, slot);
        if ((rc = hipGetLastError()) != hipSuccess) return rc;
        done = (size_t)((rounds * kScanWaveWindows + stride - 1) / stride); // k-mers that start before the last round's end
        if (done >= count) return hipSuccess;
    }
    // general strides, and what the kernels above leave over.  The error slot holds byte offsets relative to `kmers`, so the
    // leftover launch passes the offset it starts at.
    const size_t rest = count - done;
    const unsigned grid = grid_for(c, (rest + kBlock - 1) / kBlock);
    if (stride <= (size_t)kStagedMaxStride)
        kmer_batch_kernel<true><<<grid, kBlock, 0, c->stream>>>(kmers + done * stride, (unsigned)k, stride, rest, o + done, slot, done * stride);
    else
        kmer_batch_kernel<false><<<grid, kBlock, 0, c->stream>>>(kmers + done * stride, (unsigned)k, stride, rest, o + done, slot, done * stride);
    return hipGetLastError();
}

// ---- the windows the matrix-core rounds leave to single threads in front of them (`skip`; the kernels' tails take those behind the last whole round)
// ASCII input at any alignment: the rounds start at the first 16-byte aligned base
inline unsigned ascii_skip(const uint8_t *ref) { return (unsigned)((16 - (reinterpret_cast<uintptr_t>(ref) & 15)) & 15); }
// packed words, 8-byte aligned (checked by the callers): words at 8 mod 16 start the rounds one word later
inline unsigned packed_skip(const uint64_t *words) { return aligned16(words) ? 0u : 32u; }

// ---- the two kinds of query of the hit lists, the multi-query count and the best match: an exact query (uint64_t) or a pattern (bitnuc_pattern).  The
// launchers and host loops below are templates over the ABI's type HQ; the kernels take its device twin (QueryKind, scan_mfma_device.h).
static_assert(sizeof(bitnuc_pattern) == sizeof(PatternSets) && alignof(bitnuc_pattern) == alignof(PatternSets), "bitnuc_pattern is PatternSets");
template <class HQ> struct DevQuery;
template <> struct DevQuery<uint64_t> { using type = unsigned long long; };
template <> struct DevQuery<bitnuc_pattern> { using type = PatternSets; };
template <class HQ> const typename DevQuery<HQ>::type *dev_queries(const HQ *q) { return reinterpret_cast<const typename DevQuery<HQ>::type *>(q); }
inline unsigned long long dev_query(uint64_t q) { return q; }
inline PatternSets dev_query(const bitnuc_pattern &p) { return *dev_queries(&p); }
template <class HQ> constexpr uintptr_t query_mask() { return sizeof(HQ) == 8 ? 7 : 3; } // a queries array's alignment: 8 bytes exact, 4 bytes patterns

// the four-channel table of the distance bytes (the scan, the hit lists): no threshold, the accumulators start at the 2^23 pack bias
template <class DQ>
inline CountMfmaTable scan_seg_table(const DQ &query, size_t k) {
    CountMfmaTable ct;
    count_mfma_table(query, k, &ct);
    for (int j = 0; j < 4; ++j) ct.c[j] = kPackBias;
    return ct;
}

// ---- the scan and its fused count: the shipped tilings, at the trip length / workgroup size / grid the caller picks
// the segment tiling (four channels per base)
template <int U, int BLOCK>
hipError_t scan_seg_t(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist, unsigned long long *slot) {
    const CountMfmaTable ct = scan_seg_table(query, k);
    kmer_scan_seg_mfma_kernel<3, U, BLOCK><<<(unsigned)(scan_rounds(n) / ((BLOCK / 64) * U) + 1), BLOCK, 0, c->stream>>>(ref, n, (unsigned)k, query, dist, slot, ct);
    return hipGetLastError();
}

// rounds of 992 windows (kmer_scan_kernel); the grid assumes `unroll` rounds per wave
template <bool AL, bool NL, bool NS, int U>
hipError_t scan992_t(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist, unsigned long long *slot, int kb, int unroll) {
    uint32_t ql, qh;
    query_planes(query, k, &ql, &qh);
    const unsigned long long rounds = n >= 1024 ? (n - 1024) / kScanWaveWindows + 1 : 0;
    kmer_scan_kernel<AL, NL, NS, U><<<grid_for(c, rounds / ((kb / 64) * unroll) + 1, kb), kb, 0, c->stream>>>(ref, n, (unsigned)k, query, ql, qh, dist, slot);
    return hipGetLastError();
}

// a ticketed count's grid: one workgroup per `per_wg` rounds, at most per_cu workgroups per CU (each arrives once at the accumulator and the ticket)
unsigned bounded_grid(const bitnuc_ctx *c, unsigned long long rounds, unsigned long long per_wg, int per_cu) {
    const unsigned long long want = rounds / per_wg + 1, cap = (unsigned long long)c->num_cu * (unsigned)per_cu;
    return (unsigned)(want < cap ? want : cap);
}

// the fused count with three channels per base: a bounded grid of per_cu workgroups per CU
template <int U>
hipError_t count3_t(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, unsigned long long *res, unsigned long long *slot, int per_cu) {
    Count3MfmaTable c3;
    count3_mfma_table(query, k, tau, &c3);
    kmer_count3_mfma_kernel<U, true><<<bounded_grid(c, scan_rounds(n), (kBlock / 64) * U, per_cu), kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, tau, res, c->d_acc + 5, c->d_tickets + 2, slot, c3);
    return hipGetLastError();
}

// the fused count on the bit-plane scan: a resident grid (the accumulator's ticket needs every workgroup to arrive; 4 trips of 4 rounds per wave keep the tail short)
template <bool AL, bool NL, int U, int GEN>
hipError_t count_scan2_t(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, unsigned long long *res, unsigned long long *slot) {
    uint32_t ql, qh;
    query_planes(query, k, &ql, &qh);
    kmer_scan2_kernel<AL, NL, false, U, true, GEN><<<bounded_grid(c, scan_rounds(n), (kBlock / 64) * 4, 8), kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, ql, qh, tau, nullptr, res, c->d_acc + 5, c->d_tickets + 2, slot);
    return hipGetLastError();
}

#ifdef BITNUC_SWEEP_VARIANTS
#include "evidence/kmer_launch.h" // the formulations that lost their A/B: the hooks below
#endif

hipError_t launch_batch(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, size_t count, uint64_t *out,
                        unsigned long long *slot) {
    unsigned long long *o = reinterpret_cast<unsigned long long *>(out);
    BITNUC_EVIDENCE(if (evidence::wants_batch(c)) return batch_legs(c, kmers, k, stride, count, o, slot, evidence::KnobLegs(c));)
    return batch_legs(c, kmers, k, stride, count, o, slot, ShippedLegs{});
}

hipError_t launch_scan(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist,
                       unsigned long long *slot) {
    const bool al = aligned16(ref) && aligned16(dist);
    BITNUC_EVIDENCE(if (evidence::wants_scan(c, al)) return evidence::launch_scan(c, ref, n, k, query, dist, slot);)
    // The contraction on the matrix cores in the tiling the fused count introduced -- a column is a segment of 32 windows, a row one of its 32
    // shifts: four MFMAs per 1024 windows -- one trip of 4 rounds per wave (the dispatcher walks the trips), one-hot operands through a wave-private LDS strip,
    // 2^23 bias + row scales for the byte pack, two v_permlane32_swap put the packed dwords in store order, nt loads and stores (scan_mfma_device.h:
    // kmer_scan_seg_mfma_kernel; profiles/r05_ab_scan_seg.txt against the natural-layout tiling's six MFMAs, which shipped first).
    // Workgroups of ONE wave (the strips are wave-private, nothing is shared inside a workgroup): 19 waves fit a CU's LDS instead of 16, and the dispatcher
    // refills a CU wave by wave (profiles/r05_ab_scan_block.txt: 1 % faster from idle than workgroups of four waves)
    if (al) return scan_seg_t<kScanSegRounds, kScanSegBlock>(c, ref, n, k, query, dist, slot);
    // unaligned pointers: rounds of 992 windows with unaligned 16-byte loads
    return scan992_t<false, false, false, 1>(c, ref, n, k, query, dist, slot, kKmerBlock, kScanUnroll);
}

// the fused count of windows with d <= tau into *res
hipError_t launch_count(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, unsigned long long *res,
                        unsigned long long *slot) {
    const bool al = aligned16(ref);
    BITNUC_EVIDENCE(if (evidence::wants_count(c, al)) return evidence::launch_count(c, ref, n, k, query, tau, res, slot);)
    // scan_mfma_device.h: kmer_count3_mfma_kernel: segments of 32 windows x 32 shifts with THREE channels per base -- three MFMAs per 1024
    // windows --, the threshold inside the product (6-bit fields 32 + tau - d, three rows per register; v_or3 + v_bitop3 + v_bcnt per four windows, nothing on
    // the scalar unit), a bounded grid (one arrival per workgroup at the ticket) whose waves walk trips of four rounds and load the next trip into the registers
    // the current one has just left; 12 workgroups per CU (profiles/r05_ab_count_ch3*.txt; the four-channel form it replaced: r05_ab_count_emit*.txt).
    if (al) return count3_t<kCountRounds>(c, ref, n, k, query, tau, res, slot, kCountGrid);
    // unaligned reference pointer: the bit-plane scan with unaligned 16-byte loads
    return count_scan2_t<false, false, 1, 0>(c, ref, n, k, query, tau, res, slot);
}

// ---- the scan and its fused count on packed words (scan_packed_device.h).  The tail threads take the first packed_skip windows, so both alignments
// run the same kernel.
hipError_t launch_scan_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, uint64_t query, uint8_t *dist) {
    PackedScanTable t;
    scan_packed_table(query, k, &t);
    const unsigned skip = packed_skip(words);
    packed_scan_mfma_kernel<<<(unsigned)(scan_rounds(n, skip) / 4 + 1), kPackedBlockScan, 0, c->stream>>>(words, n, skip, (unsigned)k, query, dist, t);
    return hipGetLastError();
}

// a bounded grid of kCountGrid workgroups per CU, as the ASCII count; its own accumulator and ticket (d_acc[6], d_tickets[3])
hipError_t launch_count_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, uint64_t query, unsigned tau, unsigned long long *res) {
    Count3MfmaTable t;
    count3_packed_table(query, k, tau, &t);
    const unsigned skip = packed_skip(words);
    packed_count3_mfma_kernel<<<bounded_grid(c, scan_rounds(n, skip), (kBlock / 64) * 4, kCountGrid), kBlock, 0, c->stream>>>(words, n, skip, (unsigned)k, query, tau, res, c->d_acc + 6, c->d_tickets + 3, t);
    return hipGetLastError();
}

// no windows: nothing of the reference is looked at, the outputs get the family's fill
inline bool no_windows(size_t n, size_t k) { return k == 0 || n < k; }

// the single-query packed scan's and count's argument checks, in the header's order: k, the word count, no windows (*none), then the words (the
// searches of ref_dispatch.h look at the words after their own arguments: the two orders answer alike)
int check_packed(const void *words, size_t n_words, size_t n, size_t k, bool *none, bitnuc_err *err) {
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (n_words < words_for(n)) return fail(err, BITNUC_INVALID_LENGTH, n);
    *none = no_windows(n, k);
    if (*none) return BITNUC_OK;
    if (!words || (reinterpret_cast<uintptr_t>(words) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// ---- the hit lists (scan_hits_device.h): count pass, scan of the per-trip counts, emit pass.  Context scratch 7 holds the counts (one u32 per trip, the
// head's and the tail's) and the tiles' offsets; a launch recorded into a hipGraph keeps it (ensure_scratch).  cap == 0 skips the emit pass.  pos_base is added to every
// position (the host forms' chunk offset).
template <class HQ> struct HitsArgsT { HQ query; unsigned tau; unsigned long long *pos; uint8_t *hd; unsigned long long cap, *n_hits, pos_base; };
using HitsArgs = HitsArgsT<uint64_t>;

int hits_scratch(bitnuc_ctx *c, unsigned long long ntr, unsigned **counts, unsigned long long **tiles, bitnuc_err *err) {
    const unsigned long long ntiles = (ntr + kHitsTile - 1) / kHitsTile, cbytes = (4 * ntr + 255) & ~255ull;
    if (int st = ensure_scratch(c, 7, cbytes + 8 * ntiles, err)) return st;
    *counts = reinterpret_cast<unsigned *>(c->scratch[7]);
    *tiles = reinterpret_cast<unsigned long long *>(c->scratch[7] + cbytes);
    return BITNUC_OK;
}

hipError_t hits_scan(bitnuc_ctx *c, unsigned *counts, unsigned long long ntr, unsigned long long *tiles, unsigned long long *n_hits) {
    const unsigned long long ntiles = (ntr + kHitsTile - 1) / kHitsTile;
    hits_scan_tiles_kernel<<<(unsigned)ntiles, kHitsTileBlock, 0, c->stream>>>(counts, ntr, tiles);
    hits_scan_top_kernel<<<1, kHitsTopBlock, 0, c->stream>>>(tiles, ntiles, n_hits);
    return hipGetLastError();
}

// d_ref at any alignment (ascii_skip): the windows before the rounds are the first workgroup's
template <class HQ>
int launch_hits(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const HitsArgsT<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    using DQ = typename DevQuery<HQ>::type;
    const DQ query = dev_query(a.query);
    const unsigned skip = ascii_skip(ref);
    const unsigned long long ntr = hits_trips(n, skip) + 2;
    unsigned *counts;
    unsigned long long *tiles;
    if (int st = hits_scratch(c, ntr, &counts, &tiles, err)) return st;
    const CountMfmaTable ct = scan_seg_table(query, k);
    kmer_hits_mfma_kernel<false, DQ><<<(unsigned)ntr, 64, 0, c->stream>>>(ref, n, skip, (unsigned)k, query, a.tau, counts, nullptr, nullptr, nullptr, 0, 0, slot, ct);
    HIPCHK(hits_scan(c, counts, ntr, tiles, a.n_hits));
    if (a.cap) kmer_hits_mfma_kernel<true, DQ><<<(unsigned)ntr, 64, 0, c->stream>>>(ref, n, skip, (unsigned)k, query, a.tau, counts, tiles, a.pos, a.hd, a.cap, a.pos_base, slot, ct);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// d_words 8-byte aligned (packed_skip)
template <class HQ>
int launch_hits_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, const HitsArgsT<HQ> &a, bitnuc_err *err) {
    using DQ = typename DevQuery<HQ>::type;
    const DQ query = dev_query(a.query);
    const unsigned skip = packed_skip(words);
    const unsigned long long ntr = hits_trips(n, skip) + 2;
    unsigned *counts;
    unsigned long long *tiles;
    if (int st = hits_scratch(c, ntr, &counts, &tiles, err)) return st;
    PackedScanTable t;
    scan_packed_table(query, k, &t);
    packed_hits_mfma_kernel<false, DQ><<<(unsigned)ntr, 64, 0, c->stream>>>(words, n, skip, (unsigned)k, query, a.tau, counts, nullptr, nullptr, nullptr, 0, 0, t);
    HIPCHK(hits_scan(c, counts, ntr, tiles, a.n_hits));
    if (a.cap) packed_hits_mfma_kernel<true, DQ><<<(unsigned)ntr, 64, 0, c->stream>>>(words, n, skip, (unsigned)k, query, a.tau, counts, tiles, a.pos, a.hd, a.cap, a.pos_base, t);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// the hit calls' output checks (after the count's / packed count's checks of k, lengths and words): n_hits and pos 8-byte aligned, pos NULL only for cap 0
int check_hits_out(const void *pos, size_t cap, const void *n_hits, bitnuc_err *err) {
    if (!n_hits || (reinterpret_cast<uintptr_t>(n_hits) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    if ((!pos && cap) || (reinterpret_cast<uintptr_t>(pos) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// The host forms' chunk loop: the input chunk in scratch 0, the chunk's positions / distances in scratch 1 / 2 (at most the cap still open), its
// count in scratch 3.  `launch(i0, m, a)` runs the windows [i0, i0 + m) with a's outputs; positions come back shifted by i0.  Stops at the first
// failing chunk (drain: its first invalid byte, relative to the whole sequence through the slot's base).
template <class HQ, class Launch>
int hits_host_loop(bitnuc_ctx *c, size_t nwin, size_t per, unsigned tau, const HQ &query, uint64_t *pos, uint8_t *hit_dist, size_t cap, uint64_t *n_hits,
                   bitnuc_err *err, Launch launch) {
    const size_t pcap = cap < per ? cap : per;
    if (pcap) {
        if (int st = ensure_scratch(c, 1, pcap * 8, err)) return st;
        if (hit_dist) if (int st = ensure_scratch(c, 2, pcap, err)) return st;
    }
    if (int st = ensure_scratch(c, 3, 64, err)) return st;
    uint64_t total = 0;
    for (size_t i0 = 0; i0 < nwin; i0 += per) {
        const size_t m = nwin - i0 < per ? nwin - i0 : per;
        const size_t open = total < cap ? cap - total : 0, ccap = open < m ? open : m;
        const HitsArgsT<HQ> a{query, tau, reinterpret_cast<unsigned long long *>(c->scratch[1]), hit_dist ? c->scratch[2] : nullptr, ccap,
                         reinterpret_cast<unsigned long long *>(c->scratch[3]), i0};
        if (int st = launch(i0, m, a)) return st;
        uint64_t part = 0;
        HIPCHK(hipMemcpyAsync(&part, c->scratch[3], 8, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        const size_t got = part < ccap ? (size_t)part : ccap;
        if (got) {
            HIPCHK(hipMemcpyAsync(pos + total, c->scratch[1], got * 8, hipMemcpyDeviceToHost, c->stream));
            if (hit_dist) HIPCHK(hipMemcpyAsync(hit_dist + total, c->scratch[2], got, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        total += part;
    }
    *n_hits = total;
    return BITNUC_OK;
}

// ---- the count for many queries (scan_multi_device.h).  Context scratch 8 holds the tables (one Count3MfmaTable per query, built in-stream from d_queries /
// d_taus); a launch recorded into a hipGraph keeps it (ensure_scratch: warm up with the same n_queries before capturing).  counts[] is zeroed first in the
// same stream, then every workgroup adds its per-query sums.  The grid: kMultiGrid workgroups per CU at most (one fits a CU's LDS) x the query blocks.
constexpr int kMultiGrid = 1;

template <class HQ> struct MultiArgsT { const HQ *queries; const uint32_t *taus; size_t nq; unsigned long long *counts; };
using MultiArgs = MultiArgsT<uint64_t>;

template <bool PACKED, class HQ>
int multi_setup(bitnuc_ctx *c, size_t k, const MultiArgsT<HQ> &a, unsigned long long rounds, const Count3MfmaTable **tabs, dim3 *grid, bitnuc_err *err) {
    if (int st = ensure_scratch(c, 8, a.nq * sizeof(Count3MfmaTable), err)) return st;
    Count3MfmaTable *t = reinterpret_cast<Count3MfmaTable *>(c->scratch[8]);
    HIPCHK(hipMemsetAsync(a.counts, 0, a.nq * sizeof(uint64_t), c->stream));
    count3_tables_kernel<PACKED><<<(unsigned)a.nq, 64, 0, c->stream>>>(dev_queries(a.queries), a.taus, (unsigned)k, t);
    HIPCHK(hipGetLastError());
    *tabs = t;
    *grid = dim3(bounded_grid(c, rounds, (kMultiBlock / 64) * kMultiRounds, kMultiGrid), (unsigned)((a.nq + kMultiQB - 1) / kMultiQB), 1);
    return BITNUC_OK;
}

// d_ref at any alignment (ascii_skip)
template <class HQ>
int launch_count_multi(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const MultiArgsT<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    const unsigned skip = ascii_skip(ref);
    const Count3MfmaTable *tabs;
    dim3 grid;
    if (int st = multi_setup<false>(c, k, a, scan_rounds(n, skip), &tabs, &grid, err)) return st;
    kmer_count3_multi_kernel<kMultiRounds><<<grid, kMultiBlock, 0, c->stream>>>(ref, n, skip, (unsigned)k, dev_queries(a.queries), a.taus, (unsigned)a.nq, tabs,
                                                                               a.counts, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// d_words 8-byte aligned (packed_skip)
template <class HQ>
int launch_count_multi_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, const MultiArgsT<HQ> &a, bitnuc_err *err) {
    const unsigned skip = packed_skip(words);
    const Count3MfmaTable *tabs;
    dim3 grid;
    if (int st = multi_setup<true>(c, k, a, scan_rounds(n, skip), &tabs, &grid, err)) return st;
    packed_count3_multi_kernel<<<grid, kMultiBlock, 0, c->stream>>>(words, n, skip, (unsigned)k, dev_queries(a.queries), a.taus, (unsigned)a.nq, tabs, a.counts);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// the multi-query calls' checks 4 - 6 (after ctx, k and the packed word count): n_queries == 0 -> OK (*none), too many queries, the three arrays
// (qmask: 7 for exact queries, 3 for patterns)
int check_multi(const void *queries, const void *taus, size_t nq, const void *counts, bool *none, bitnuc_err *err, uintptr_t qmask) {
    *none = nq == 0;
    if (*none) return BITNUC_OK;
    if (nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, nq);
    if (!counts || (reinterpret_cast<uintptr_t>(counts) & 7) || !queries || (reinterpret_cast<uintptr_t>(queries) & qmask) || !taus ||
        (reinterpret_cast<uintptr_t>(taus) & 3))
        return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// windows x queries, saturated: what the host forms' cutoff is judged on
inline size_t multi_work(size_t nwin, size_t nq) { return nwin > (size_t)-1 / nq ? (size_t)-1 : nwin * nq; }

// The host forms' chunk loop: queries and thresholds copied once into scratch 2, the chunk's counts in scratch 1; `launch(i0, a)` runs the chunk of
// windows starting at i0 with a's device arrays.  Sums per query; stops at the first failing chunk (drain: its first invalid byte).
template <class HQ, class Launch>
int multi_host_loop(bitnuc_ctx *c, size_t nwin, size_t per, const HQ *queries, const uint32_t *taus, size_t nq, uint64_t *counts, bitnuc_err *err,
                    Launch launch) {
    constexpr size_t qb = sizeof(HQ); // 8: exact queries, 16: patterns
    if (int st = ensure_scratch(c, 1, nq * 8, err)) return st;
    if constexpr (qb == 8) {
        if (int st = ensure_scratch(c, 2, nq * 12, err)) return st;
    } else {
        if (int st = ensure_scratch(c, 2, nq * (qb + 4), err)) return st;
    }
    HIPCHK(hipMemcpyAsync(c->scratch[2], queries, nq * qb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->scratch[2] + nq * qb, taus, nq * 4, hipMemcpyHostToDevice, c->stream));
    const MultiArgsT<HQ> a{reinterpret_cast<const HQ *>(c->scratch[2]), reinterpret_cast<const uint32_t *>(c->scratch[2] + nq * qb), nq,
                           reinterpret_cast<unsigned long long *>(c->scratch[1])};
    std::vector<uint64_t> part(nq), total(nq, 0);
    for (size_t i0 = 0; i0 < nwin; i0 += per) {
        if (int st = launch(i0, a)) return st;
        HIPCHK(hipMemcpyAsync(part.data(), c->scratch[1], nq * 8, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        for (size_t q = 0; q < nq; ++q) total[q] += part[q];
    }
    memcpy(counts, total.data(), nq * 8);
    return BITNUC_OK;
}

// ---- the best match per query (scan_best_device.h).  Context scratch 9 holds the keys (one u64 per query, all-ones = no window yet) and behind them the
// tables (one BestTable per query, built in-stream from d_queries); a launch recorded into a hipGraph keeps it (ensure_scratch: warm up with the same
// n_queries before capturing).  The keys are set to all-ones first in the same stream, every workgroup then takes its per-query minima into them and
// best_finish_kernel writes pos[] / dist[].  The grid: the multi-query count's (one workgroup per CU at most x the query blocks).
template <class HQ> struct BestArgsT { const HQ *queries; size_t nq; unsigned long long *pos; uint8_t *dist; };
using BestArgs = BestArgsT<uint64_t>;

template <bool PACKED, class HQ>
int best_setup(bitnuc_ctx *c, size_t k, const BestArgsT<HQ> &a, unsigned long long rounds, unsigned long long **keys, const BestTable **tabs, dim3 *grid, bitnuc_err *err) {
    const size_t kbytes = (a.nq * 8 + 255) & ~(size_t)255;
    if (int st = ensure_scratch(c, 9, kbytes + a.nq * sizeof(BestTable), err)) return st;
    *keys = reinterpret_cast<unsigned long long *>(c->scratch[9]);
    BestTable *t = reinterpret_cast<BestTable *>(c->scratch[9] + kbytes);
    HIPCHK(hipMemsetAsync(*keys, 0xFF, a.nq * sizeof(uint64_t), c->stream));
    best_tables_kernel<PACKED><<<(unsigned)a.nq, 64, 0, c->stream>>>(dev_queries(a.queries), (unsigned)k, t);
    HIPCHK(hipGetLastError());
    *tabs = t;
    *grid = dim3(bounded_grid(c, rounds, (kMultiBlock / 64) * kMultiRounds, kMultiGrid), (unsigned)((a.nq + kMultiQB - 1) / kMultiQB), 1);
    return BITNUC_OK;
}

template <class HQ>
int best_finish(bitnuc_ctx *c, const unsigned long long *keys, const BestArgsT<HQ> &a, bitnuc_err *err) {
    HIPCHK(hipGetLastError());
    best_finish_kernel<<<(unsigned)((a.nq + 255) / 256), 256, 0, c->stream>>>(keys, (unsigned)a.nq, a.pos, a.dist);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// d_ref at any alignment (ascii_skip)
template <class HQ>
int launch_best(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const BestArgsT<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    const unsigned skip = ascii_skip(ref);
    unsigned long long *keys;
    const BestTable *tabs;
    dim3 grid;
    if (int st = best_setup<false>(c, k, a, scan_rounds(n, skip), &keys, &tabs, &grid, err)) return st;
    kmer_best_kernel<kMultiRounds><<<grid, kMultiBlock, 0, c->stream>>>(ref, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, tabs, keys, slot);
    return best_finish(c, keys, a, err);
}

// d_words 8-byte aligned (packed_skip)
template <class HQ>
int launch_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, const BestArgsT<HQ> &a, bitnuc_err *err) {
    const unsigned skip = packed_skip(words);
    unsigned long long *keys;
    const BestTable *tabs;
    dim3 grid;
    if (int st = best_setup<true>(c, k, a, scan_rounds(n, skip), &keys, &tabs, &grid, err)) return st;
    packed_best_kernel<<<grid, kMultiBlock, 0, c->stream>>>(words, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, tabs, keys);
    return best_finish(c, keys, a, err);
}

// the best-match calls' checks 4 - 6 (after ctx, k and the packed word count): n_queries == 0 -> OK (*none), too many queries, the three arrays
// (qmask: 7 for exact queries, 3 for patterns)
int check_best(const void *queries, size_t nq, const void *pos, const void *dist, bool *none, bitnuc_err *err, uintptr_t qmask) {
    *none = nq == 0;
    if (*none) return BITNUC_OK;
    if (nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, nq);
    if (!pos || (reinterpret_cast<uintptr_t>(pos) & 7) || !queries || (reinterpret_cast<uintptr_t>(queries) & qmask) || !dist) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// no windows: every pos UINT64_MAX, every dist 0xFF
int best_fill_dev(bitnuc_ctx *c, uint64_t *d_pos, uint8_t *d_dist, size_t nq, bitnuc_err *err) {
    HIPCHK(hipMemsetAsync(d_pos, 0xFF, nq * sizeof(uint64_t), c->stream));
    HIPCHK(hipMemsetAsync(d_dist, 0xFF, nq, c->stream));
    return BITNUC_OK;
}

// The host forms' chunk loop: the queries copied once into scratch 2, the chunk's positions / distances in scratch 1 / 3; `launch(i0, a)` runs the chunk
// of windows starting at i0 with a's device arrays.  The chunks' results merge by the lexicographic (dist, absolute pos) minimum; stops at the first
// failing chunk (drain: its first invalid byte).
template <class HQ, class Launch>
int best_host_loop(bitnuc_ctx *c, size_t nwin, size_t per, const HQ *queries, size_t nq, uint64_t *pos, uint8_t *dist, bitnuc_err *err, Launch launch) {
    if (int st = ensure_scratch(c, 1, nq * 8, err)) return st;
    if (int st = ensure_scratch(c, 2, nq * sizeof(HQ), err)) return st;
    if (int st = ensure_scratch(c, 3, nq < 64 ? 64 : nq, err)) return st;
    HIPCHK(hipMemcpyAsync(c->scratch[2], queries, nq * sizeof(HQ), hipMemcpyHostToDevice, c->stream));
    const BestArgsT<HQ> a{reinterpret_cast<const HQ *>(c->scratch[2]), nq, reinterpret_cast<unsigned long long *>(c->scratch[1]), c->scratch[3]};
    std::vector<uint64_t> ppos(nq), bpos(nq, ~0ull);
    std::vector<uint8_t> pdist(nq), bdist(nq, 0xFF);
    for (size_t i0 = 0; i0 < nwin; i0 += per) {
        if (int st = launch(i0, a)) return st;
        HIPCHK(hipMemcpyAsync(ppos.data(), c->scratch[1], nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(pdist.data(), c->scratch[3], nq, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        for (size_t q = 0; q < nq; ++q) // chunks come in ascending order: a later chunk wins on a smaller distance only
            if (pdist[q] < bdist[q]) bdist[q] = pdist[q], bpos[q] = i0 + ppos[q];
    }
    memcpy(pos, bpos.data(), nq * 8);
    memcpy(dist, bdist.data(), nq);
    return BITNUC_OK;
}

// ---- the mismatch histogram per query (scan_hist_device.h).  The tables are the best match's and live where its tables live, in context scratch 9 (behind
// the space of its keys: the two calls run in stream order, as the two users of scratch 7 do); a launch recorded into a hipGraph keeps it (ensure_scratch:
// warm up with the same n_queries before capturing).  hist[] is zeroed first in the same stream, then every workgroup adds its per-(query, bin) sums.  The
// grid: the best match's.  n_bins <= 8 runs the one-tier kernels, 9 - 16 the two-tier ones.
template <class HQ> struct HistArgsT { const HQ *queries; size_t nq, n_bins; unsigned long long *hist; };
static_assert(BITNUC_HIST_MAX_BINS == kHistMaxBins, "the kernels' two tiers of eight bins");

template <bool PACKED, class HQ>
int hist_setup(bitnuc_ctx *c, size_t k, const HistArgsT<HQ> &a, unsigned long long rounds, const BestTable **tabs, dim3 *grid, bitnuc_err *err) {
    const size_t kbytes = (a.nq * 8 + 255) & ~(size_t)255;
    if (int st = ensure_scratch(c, 9, kbytes + a.nq * sizeof(BestTable), err)) return st;
    BestTable *t = reinterpret_cast<BestTable *>(c->scratch[9] + kbytes);
    HIPCHK(hipMemsetAsync(a.hist, 0, a.nq * a.n_bins * sizeof(uint64_t), c->stream));
    best_tables_kernel<PACKED><<<(unsigned)a.nq, 64, 0, c->stream>>>(dev_queries(a.queries), (unsigned)k, t);
    HIPCHK(hipGetLastError());
    *tabs = t;
    *grid = dim3(bounded_grid(c, rounds, (kMultiBlock / 64) * kMultiRounds, kMultiGrid), (unsigned)((a.nq + kMultiQB - 1) / kMultiQB), 1);
    return BITNUC_OK;
}

// d_ref at any alignment (ascii_skip)
template <class HQ>
int launch_hist(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const HistArgsT<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    const unsigned skip = ascii_skip(ref);
    const BestTable *tabs;
    dim3 grid;
    if (int st = hist_setup<false>(c, k, a, scan_rounds(n, skip), &tabs, &grid, err)) return st;
    if (a.n_bins <= 8)
        kmer_hist_kernel<kMultiRounds, 1><<<grid, kMultiBlock, 0, c->stream>>>(ref, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, (unsigned)a.n_bins, tabs,
                                                                            a.hist, slot);
    else
        kmer_hist_kernel<kMultiRounds, 2><<<grid, kMultiBlock, 0, c->stream>>>(ref, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, (unsigned)a.n_bins, tabs,
                                                                            a.hist, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// d_words 8-byte aligned (packed_skip)
template <class HQ>
int launch_hist_packed(bitnuc_ctx *c, const uint64_t *words, size_t n, size_t k, const HistArgsT<HQ> &a, bitnuc_err *err) {
    const unsigned skip = packed_skip(words);
    const BestTable *tabs;
    dim3 grid;
    if (int st = hist_setup<true>(c, k, a, scan_rounds(n, skip), &tabs, &grid, err)) return st;
    if (a.n_bins <= 8)
        packed_hist_kernel<1><<<grid, kMultiBlock, 0, c->stream>>>(words, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, (unsigned)a.n_bins, tabs, a.hist);
    else
        packed_hist_kernel<2><<<grid, kMultiBlock, 0, c->stream>>>(words, n, skip, (unsigned)k, dev_queries(a.queries), (unsigned)a.nq, (unsigned)a.n_bins, tabs, a.hist);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// the histogram calls' checks 4 - 7 (after ctx, k and the packed word count): the number of bins, n_queries == 0 -> OK (*none), too many queries, the two
// arrays (qmask: 7 for exact queries, 3 for patterns)
int check_hist(const void *queries, size_t nq, size_t n_bins, const void *hist, bool *none, bitnuc_err *err, uintptr_t qmask) {
    *none = false;
    if (n_bins == 0 || n_bins > BITNUC_HIST_MAX_BINS) return fail(err, BITNUC_UNSUPPORTED, n_bins);
    *none = nq == 0;
    if (*none) return BITNUC_OK;
    if (nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, nq);
    if (!hist || (reinterpret_cast<uintptr_t>(hist) & 7) || !queries || (reinterpret_cast<uintptr_t>(queries) & qmask)) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}
// the queries as the host code takes them (scan_hist_host.h: window_dist's two kinds)
inline const uint64_t *host_queries(const uint64_t *q) { return q; }
inline const PatternSets *host_queries(const bitnuc_pattern *q) { return reinterpret_cast<const PatternSets *>(q); }

// The host forms' chunk loop: the queries copied once into scratch 2, the chunk's histogram in scratch 1; `launch(i0, a)` runs the chunk of windows starting
// at i0 with a's device arrays.  Sums per bin; stops at the first failing chunk (drain: its first invalid byte).
template <class HQ, class Launch>
int hist_host_loop(bitnuc_ctx *c, size_t nwin, size_t per, const HQ *queries, size_t nq, size_t n_bins, uint64_t *hist, bitnuc_err *err, Launch launch) {
    const size_t cells = nq * n_bins;
    if (int st = ensure_scratch(c, 1, cells * 8, err)) return st;
    if (int st = ensure_scratch(c, 2, nq * sizeof(HQ), err)) return st;
    HIPCHK(hipMemcpyAsync(c->scratch[2], queries, nq * sizeof(HQ), hipMemcpyHostToDevice, c->stream));
    const HistArgsT<HQ> a{reinterpret_cast<const HQ *>(c->scratch[2]), nq, n_bins, reinterpret_cast<unsigned long long *>(c->scratch[1])};
    std::vector<uint64_t> part(cells), total(cells, 0);
    for (size_t i0 = 0; i0 < nwin; i0 += per) {
        if (int st = launch(i0, a)) return st;
        HIPCHK(hipMemcpyAsync(part.data(), c->scratch[1], cells * 8, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        for (size_t i = 0; i < cells; ++i) total[i] += part[i];
    }
    memcpy(hist, total.data(), cells * 8);
    return BITNUC_OK;
}

// host-pointer packed calls: chunks of whole words; chunk w0 holds the windows [32 w0, 32 (w0 + cw)) and the k - 1 bases after them (one more word)
constexpr size_t kPackedChunkWords = kHostChunk / 32;
struct PackedChunk { size_t w0, words, bases, nwin; };
inline PackedChunk packed_chunk(size_t w0, size_t n, size_t k) {
    const size_t first = 32 * w0, nwin = n - k + 1;
    const size_t w = nwin - first < 32 * kPackedChunkWords ? nwin - first : 32 * kPackedChunkWords;
    const size_t bases = w + k - 1;
    return PackedChunk{w0, words_for(bases), bases, w};
}

// ---- host-pointer k-mer calls: jobs of host_pipe.h ---------------------------------------------------------------------------
// The drop-in forms of configs 3 and 5 for a caller whose data lives in host memory (README.md:52-56's host loop over as_2bit;
// the window idiom of src/lib.rs:170-173): PCIe-bound, so the point is to keep both DMA engines busy -- round 2's simple path
// (one pageable hipMemcpyAsync in, kernel, one out, host wait, per 128 MiB chunk) left each idle two thirds of the time.
// Errors: one slot per chunk with the chunk's byte offset as index base, so the first invalid examined byte of the whole call is
// reported; `out` past it is unspecified.
struct BatchJob { // items are k-mers
    bitnuc_ctx *c; const uint8_t *kmers; size_t k, stride, count; uint64_t *out;
    int in_kind, out_kind; // the side that moves more bytes per k-mer (8 out against `stride` in) gets the large (A) buffers
    static constexpr bool drains = true, inout = false;
    BatchJob(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, size_t count, uint64_t *out)
        : c(c), kmers(kmers), k(k), stride(stride), count(count), out(out), in_kind(stride >= 8 ? kBufA : kBufB), out_kind(stride >= 8 ? kBufB : kBufA) {}
    size_t pipe_per(size_t chunk) const { // as many k-mers as fit BOTH buffers (A: chunk, B: chunk / 4)
        const size_t in_cap = in_kind == kBufA ? chunk : chunk / 4, out_cap = out_kind == kBufA ? chunk : chunk / 4;
        size_t per = out_cap / 8;                                           // words that fit the output buffer
        const size_t by_bytes = in_cap > k ? (in_cap - k) / stride + 1 : 1; // k-mers whose bytes fit the input buffer
        if (by_bytes < per) per = by_bytes;
        if (per >= 1024) per &= ~(size_t)1023; // whole dense items / window rounds per chunk where the chunk is large enough to care
        return per == 0 ? 1 : per;
    }
    size_t scratch_per() const { return kHostChunk / stride; } // a chunk stays <= kHostChunk bytes
    const void *in_src(size_t i0) const { return kmers + i0 * stride; }
    size_t in_bytes(size_t m) const { return (m - 1) * stride + k; }
    void *out_dst(size_t i0) const { return out + i0; }
    size_t out_bytes(size_t m) const { return m * 8; }
    int launch(size_t i0, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err) const {
        unsigned long long *slot;
        if (int st = take_slot(c, (unsigned long long)i0 * stride, &slot, err)) return st;
        HIPCHK(launch_batch(c, d_in, k, stride, m, reinterpret_cast<uint64_t *>(d_out), slot));
        return BITNUC_OK;
    }
};

// items are windows: windows [i0, i0 + m) need bases [i0, i0 + m + k - 1), consecutive chunks overlap by the k - 1 halo bases
struct ScanJob {
    bitnuc_ctx *c; const uint8_t *ref; size_t count, k; uint64_t query; uint8_t *dist;
    static constexpr int in_kind = kBufA, out_kind = kBufC; // input AND output are a byte per window
    static constexpr bool drains = true, inout = false;
    size_t pipe_per(size_t chunk) const { return chunk; } // chunk windows + 31 halo bases fit chunk + 64
    size_t scratch_per() const { return kHostChunk; }
    const void *in_src(size_t i0) const { return ref + i0; }
    size_t in_bytes(size_t m) const { return m + k - 1; }
    void *out_dst(size_t i0) const { return dist + i0; }
    size_t out_bytes(size_t m) const { return m; }
    int launch(size_t i0, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err) const {
        unsigned long long *slot;
        if (int st = take_slot(c, i0, &slot, err)) return st;
        HIPCHK(launch_scan(c, d_in, in_bytes(m), k, query, d_out, slot));
        return BITNUC_OK;
    }
};

// ---- the chunks of an indel-tolerant walk along a reference and the bounded grid that walks them (scan_edist_ref_device.h), for the two launchers
// below.  `lead`: the columns at the start of the buffer that are run but not reported (the host chunk loops' overlap): at most kEdistRefLead and,
// packed, whole words; false for any other
struct EdistRefGrid { unsigned long long nchunks; unsigned blocks; };
template <bool PACKED>
bool edist_ref_grid(const bitnuc_ctx *c, size_t n, size_t lead, EdistRefGrid &g) {
    if (lead >= n || lead > kEdistRefLead || (PACKED && lead % 32)) return false;
    g.nchunks = (n - lead + kEdistRefChunk - 1) / kEdistRefChunk;
    const unsigned long long want = (g.nchunks + kEdistRefBlock - 1) / kEdistRefBlock, bound = (unsigned long long)c->num_cu * kEdistRefBlocksPerCu;
    g.blocks = (unsigned)(want < bound ? want : bound);
    return true;
}

// ---- the indel-tolerant search along a reference (scan_edist_ref_device.h): the best match and the count per query by EDIT distance, one
// launcher for both query kinds.  Context scratch 9 (the Hamming best match's, shared in stream order) holds one 8-byte key per query and
// behind them one 16-byte table per query (edist_tables_kernel: one form for both kinds); a launch recorded into a hipGraph keeps it (ensure_scratch:
// warm up with the same n_queries before capturing).  `lead` as edist_ref_grid takes it; the best match's ends come back counted from column `lead`.
template <bool PACKED, bool COUNT, class HQ>
int launch_kmer_edist(bitnuc_ctx *c, const void *data, size_t n, size_t lead, size_t k, const HQ *d_queries, const uint32_t *d_taus, size_t nq,
                      unsigned long long *out, uint8_t *dist, unsigned long long *slot, bitnuc_err *err) {
    EdistRefGrid g;
    if (!edist_ref_grid<PACKED>(c, n, lead, g)) return fail(err, BITNUC_UNSUPPORTED, lead);
    const size_t kbytes = (nq * 8 + 255) & ~(size_t)255;
    if (int st = ensure_scratch(c, 9, kbytes + nq * kEdistEntry, err)) return st;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(c->scratch[9]);
    u32x4 *tabs = reinterpret_cast<u32x4 *>(c->scratch[9] + kbytes);
    if constexpr (COUNT) HIPCHK(hipMemsetAsync(out, 0, nq * sizeof(uint64_t), c->stream));
    else HIPCHK(hipMemsetAsync(keys, 0xFF, nq * sizeof(uint64_t), c->stream));
    edist_tables_kernel<<<(unsigned)((nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)nq, (unsigned)k, tabs);
    HIPCHK(hipGetLastError());
    kmer_edist_kernel<PACKED, COUNT><<<g.blocks, kEdistRefBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(data), (unsigned long long)n, (unsigned)lead, (unsigned)k, (unsigned)nq, tabs, d_taus, COUNT ? out : keys, slot);
    HIPCHK(hipGetLastError());
    if constexpr (!COUNT) {
        edist_ref_finish_kernel<<<(unsigned)((nq + 255) / 256), 256, 0, c->stream>>>(keys, (unsigned)nq, (unsigned long long)lead, out, dist);
        HIPCHK(hipGetLastError());
    }
    return BITNUC_OK;
}

// ---- the indel-tolerant hit list (scan_edist_hits_device.h): count pass per chunk of kEdistRefChunk ends, the Hamming hit list's scan over the chunks'
// counts, emit pass.  Context scratch 7 (the Hamming hit list's, shared in stream order) holds the scanned counts, the tiles' offsets and, behind them,
// the raw counts; a launch recorded into a hipGraph keeps it (ensure_scratch).  The query's table entry is built here and passed by value.  `lead` as
// edist_ref_grid takes it; a.pos_base is the end of the first reported column minus one.
template <bool PACKED, class HQ>
int launch_edist_hits(bitnuc_ctx *c, const void *data, size_t n, size_t lead, size_t k, const HitsArgsT<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    EdistRefGrid g;
    if (!edist_ref_grid<PACKED>(c, n, lead, g)) return fail(err, BITNUC_UNSUPPORTED, lead);
    const unsigned long long nch = g.nchunks, ntiles = (nch + kHitsTile - 1) / kHitsTile;
    const unsigned long long cbytes = (4 * nch + 255) & ~255ull, tbytes = (8 * ntiles + 255) & ~255ull;
    if (int st = ensure_scratch(c, 7, 2 * cbytes + tbytes, err)) return st;
    unsigned *counts = reinterpret_cast<unsigned *>(c->scratch[7]);
    unsigned long long *tiles = reinterpret_cast<unsigned long long *>(c->scratch[7] + cbytes);
    unsigned *raw = reinterpret_cast<unsigned *>(c->scratch[7] + cbytes + tbytes);
    const bitnuc_host::EdistPeq p = bitnuc_host::edist_peq(dev_query(a.query), k);
    const u32x4 tab{p.m[0], p.m[1], p.m[2], p.m[3]};
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(data);
    kmer_edist_hits_kernel<PACKED, false><<<g.blocks, kEdistRefBlock, 0, c->stream>>>(bytes, (unsigned long long)n, (unsigned)lead, (unsigned)k, tab, a.tau, counts, raw,
                                                                                   nullptr, nullptr, nullptr, 0, 0, slot);
    HIPCHK(hits_scan(c, counts, nch, tiles, a.n_hits));
    if (a.cap)
        kmer_edist_hits_kernel<PACKED, true><<<g.blocks, kEdistRefBlock, 0, c->stream>>>(bytes, (unsigned long long)n, (unsigned)lead, (unsigned)k, tab, a.tau, counts, raw,
                                                                                      tiles, a.pos, a.hd, a.cap, a.pos_base, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// ---- the grid of the indel-tolerant family's second stage (scan_edist_start_device.h): one item per lane, the family's bound on the workgroups
inline unsigned start_grid(const bitnuc_ctx *c, size_t count) {
    const size_t want = (count + kEdistBlock - 1) / kEdistBlock, cap = (size_t)c->num_cu * kEdistBlocksPerCu;
    return (unsigned)(want < cap ? want : cap);
}

} // namespace

// ---- the searches along a reference: inputs, searches and the two skeletons the entry points below name
#include "ref_dispatch.h"

extern "C" {

int bitnuc_as_2bit_batch_dev(bitnuc_ctx *c, const uint8_t *d_kmers, size_t k, size_t stride, size_t count, uint64_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0) return BITNUC_OK;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k); // packing/naive.rs:5-7, before any base
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 7) || stride == 0) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (k == 0) { // as_2bit(b"") == Ok(0)
        HIPCHK(hipMemsetAsync(d_out, 0, sizeof(uint64_t) * count, c->stream));
        return BITNUC_OK;
    }
    if (!d_kmers) return fail(err, BITNUC_UNSUPPORTED);
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    HIPCHK(launch_batch(c, d_kmers, k, stride, count, d_out, slot));
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_scan_dev(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, uint8_t *d_dist, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (no_windows(n, k)) return BITNUC_OK;
    if (!d_ref || !d_dist) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    HIPCHK(launch_scan(c, d_ref, n, k, query, d_dist, slot));
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_count_dev(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_count, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (!d_count || (reinterpret_cast<uintptr_t>(d_count) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (no_windows(n, k)) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), c->stream));
        return BITNUC_OK;
    }
    if (!d_ref) return fail(err, BITNUC_UNSUPPORTED);
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    HIPCHK(launch_count(c, d_ref, n, k, query, tau, reinterpret_cast<unsigned long long *>(d_count), slot));
    return BITNUC_OK;
}

int bitnuc_hdist_dev(bitnuc_ctx *c, const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, size_t n_bases, uint32_t *d_result, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    const size_t need = words_for(n_bases);
    if (na < need || nb < need) return fail(err, BITNUC_INVALID_LENGTH, n_bases); // hamming/multi.rs:124-127
    if (!d_result) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (n_bases == 0) {
        HIPCHK(hipMemsetAsync(d_result, 0, sizeof(uint32_t), c->stream));
        return BITNUC_OK;
    }
    if (!d_a || !d_b) return fail(err, BITNUC_UNSUPPORTED);
    const unsigned long long tiles = (n_bases / 32) / (kBlock * 2) + 1;
    const unsigned grid = (unsigned)(tiles < c->hdist_blocks ? tiles : c->hdist_blocks);
    const unsigned long long *a = reinterpret_cast<const unsigned long long *>(d_a), *b = reinterpret_cast<const unsigned long long *>(d_b);
    BITNUC_EVIDENCE(if (evidence::wants_hdist(c)) return evidence::launch_hdist(c, grid, a, b, n_bases, d_result, err);)
    hdist_kernel<false><<<grid, kBlock, 0, c->stream>>>(a, b, n_bases, d_result, reinterpret_cast<unsigned *>(c->d_acc + 4), c->d_tickets + 1);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}
int bitnuc_as_2bit_batch(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, size_t count, uint64_t *out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0) return BITNUC_OK;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (!out || stride == 0) return fail(err, BITNUC_UNSUPPORTED);
    if (k == 0) { memset(out, 0, sizeof(uint64_t) * count); return BITNUC_OK; }
    if (!kmers) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    const BatchJob job(c, kmers, k, stride, count, out);
    return c->host_pipeline && (count - 1) * stride + k >= kPipeMin && stride <= ((size_t)1 << 20) ? pipe_run(c, job, err) : scratch_run(c, job, err);
}

int bitnuc_kmer_hdist_scan(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (no_windows(n, k)) return BITNUC_OK;
    if (!ref || !dist) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    const ScanJob job{c, ref, n - k + 1, k, query, dist};
    return c->host_pipeline && n >= kPipeMin ? pipe_run(c, job, err) : scratch_run(c, job, err);
}

int bitnuc_hdist(bitnuc_ctx *c, const uint64_t *a, size_t na, const uint64_t *b, size_t nb, size_t n_bases, uint32_t *out, bitnuc_err *err) {
    clear_err(err);
    const size_t need = words_for(n_bases);
    if (na < need || nb < need) return fail(err, BITNUC_INVALID_LENGTH, n_bases);
    if (!out) return fail(err, BITNUC_UNSUPPORTED);
    if (n_bases == 0) { *out = 0; return BITNUC_OK; }
    if (!a || !b) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, n_bases)) { *out = bitnuc_host::hdist_small(a, b, n_bases); return BITNUC_OK; }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    const size_t chunk_words = kHostChunk / 8;
    const size_t cw = need < chunk_words ? need : chunk_words;
    if (int st = ensure_scratch(c, 0, cw * 8, err)) return st;
    if (int st = ensure_scratch(c, 1, cw * 8, err)) return st;
    if (int st = ensure_scratch(c, 2, 64, err)) return st;
    uint32_t total = 0;
    for (size_t w0 = 0; w0 < need; w0 += cw) {
        const size_t m = need - w0 < cw ? need - w0 : cw;
        const size_t bases = (w0 + m == need) ? n_bases - w0 * 32 : m * 32;
        HIPCHK(hipMemcpyAsync(c->scratch[0], a + w0, m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->scratch[1], b + w0, m * 8, hipMemcpyHostToDevice, c->stream));
        bitnuc_err e;
        int st = bitnuc_hdist_dev(c, reinterpret_cast<const uint64_t *>(c->scratch[0]), m,
                                  reinterpret_cast<const uint64_t *>(c->scratch[1]), m, bases,
                                  reinterpret_cast<uint32_t *>(c->scratch[2]), &e);
        if (st != BITNUC_OK) { if (err) *err = e; return st; }
        uint32_t part = 0;
        HIPCHK(hipMemcpyAsync(&part, c->scratch[2], 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        total += part; // u32 wrap-around like the reference's accumulator (multi.rs:130)
    }
    *out = total;
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_scan_packed_dev(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, uint8_t *d_dist, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    bool none;
    if (int st = check_packed(d_words, n_words, n, k, &none, err)) return st;
    if (none) return BITNUC_OK;
    if (!d_dist) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    HIPCHK(launch_scan_packed(c, d_words, n, k, query, d_dist));
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_count_packed_dev(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_count,
                                       bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    bool none;
    if (int st = check_packed(d_words, n_words, n, k, &none, err)) return st;
    if (!d_count || (reinterpret_cast<uintptr_t>(d_count) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (none) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), c->stream));
        return BITNUC_OK;
    }
    HIPCHK(launch_count_packed(c, d_words, n, k, query, tau, reinterpret_cast<unsigned long long *>(d_count)));
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_scan_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, uint8_t *dist, bitnuc_err *err) {
    clear_err(err);
    bool none;
    if (int st = check_packed(words, n_words, n, k, &none, err)) return st;
    if (none) return BITNUC_OK;
    if (!dist) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, n)) { bitnuc_host::kmer_hdist_scan_packed_small(words, n, k, query, dist); return BITNUC_OK; }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    if (int st = ensure_scratch(c, 0, (kPackedChunkWords + 1) * 8, err)) return st;
    if (int st = ensure_scratch(c, 2, 32 * kPackedChunkWords, err)) return st;
    for (size_t w0 = 0; 32 * w0 < n - k + 1; w0 += kPackedChunkWords) {
        const PackedChunk ch = packed_chunk(w0, n, k);
        HIPCHK(hipMemcpyAsync(c->scratch[0], words + w0, ch.words * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_scan_packed(c, reinterpret_cast<const uint64_t *>(c->scratch[0]), ch.bases, k, query, c->scratch[2]));
        HIPCHK(hipMemcpyAsync(dist + 32 * w0, c->scratch[2], ch.nwin, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return BITNUC_OK;
}

int bitnuc_kmer_hdist_count_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *count,
                                   bitnuc_err *err) {
    clear_err(err);
    bool none;
    if (int st = check_packed(words, n_words, n, k, &none, err)) return st;
    if (!count) return fail(err, BITNUC_UNSUPPORTED);
    if (none) { *count = 0; return BITNUC_OK; }
    if (on_host(c, n)) { *count = bitnuc_host::kmer_hdist_count_packed_small(words, n, k, query, tau); return BITNUC_OK; }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    if (int st = ensure_scratch(c, 0, (kPackedChunkWords + 1) * 8, err)) return st;
    if (int st = ensure_scratch(c, 1, 64, err)) return st;
    uint64_t total = 0;
    for (size_t w0 = 0; 32 * w0 < n - k + 1; w0 += kPackedChunkWords) {
        const PackedChunk ch = packed_chunk(w0, n, k);
        HIPCHK(hipMemcpyAsync(c->scratch[0], words + w0, ch.words * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_count_packed(c, reinterpret_cast<const uint64_t *>(c->scratch[0]), ch.bases, k, query, tau, reinterpret_cast<unsigned long long *>(c->scratch[1])));
        uint64_t part = 0;
        HIPCHK(hipMemcpyAsync(&part, c->scratch[1], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        total += part;
    }
    *count = total;
    return BITNUC_OK;
}

// ---- the searches along a reference: every entry point names a skeleton, an input and a search of ref_dispatch.h --------------------------------------
// the hit lists
int bitnuc_kmer_hdist_hits_dev(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_pos, uint8_t *d_hit_dist,
                               size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistHits<uint64_t>{&query, tau, d_pos, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_hdist_hits_packed_dev(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_pos,
                                      uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistHits<uint64_t>{&query, tau, d_pos, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_hdist_hits(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *pos, uint8_t *hit_dist, size_t cap,
                           uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistHits<uint64_t>{&query, tau, pos, hit_dist, cap, n_hits}, err);
}
int bitnuc_kmer_hdist_hits_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *pos,
                                  uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistHits<uint64_t>{&query, tau, pos, hit_dist, cap, n_hits}, err);
}

// the count for many queries
int bitnuc_kmer_hdist_count_multi_dev(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, const uint32_t *d_taus, size_t n_queries,
                                      uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistCount<uint64_t>{d_queries, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_hdist_count_multi_packed_dev(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                             const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistCount<uint64_t>{d_queries, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_hdist_count_multi(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus, size_t n_queries,
                                  uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistCount<uint64_t>{queries, taus, n_queries, counts}, err);
}
int bitnuc_kmer_hdist_count_multi_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus,
                                         size_t n_queries, uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistCount<uint64_t>{queries, taus, n_queries, counts}, err);
}

// the best match per query
int bitnuc_kmer_hdist_best_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, uint64_t *d_pos,
                                 uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistBest<uint64_t>{d_queries, n_queries, d_pos, d_dist}, err);
}
int bitnuc_kmer_hdist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries,
                                        uint64_t *d_pos, uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistBest<uint64_t>{d_queries, n_queries, d_pos, d_dist}, err);
}
int bitnuc_kmer_hdist_best(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *pos, uint8_t *dist,
                           bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistBest<uint64_t>{queries, n_queries, pos, dist}, err);
}
int bitnuc_kmer_hdist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *pos,
                                  uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistBest<uint64_t>{queries, n_queries, pos, dist}, err);
}

} // extern "C"

// ---- the per-read matchers: layouts, matchers, the chunk loop, the two skeletons and the forms the entry points below name
#include "reads_dispatch.h"

extern "C" {

// ---- the per-read entry points: every form once per query kind, each naming its instantiation of the templates in reads_dispatch.h ----
// exact queries
int bitnuc_reads_hdist_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                  uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_async(c, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_hdist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries,
                                         size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_packed_async(c, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_hdist_best(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                            uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_host(c, reads, read_len, count, k, queries, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_hdist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                   uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_packed_host(c, words, read_len, count, k, queries, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_hdist_best2_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                   uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos,
                                   uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_best2_async(c, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_hdist_best2_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries,
                                          size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                          uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_best2_packed_async(c, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos,
                                    d_second_dist, err);
}
int bitnuc_reads_hdist_best2(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                             uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                             bitnuc_err *err) {
    return reads_best2_host(c, reads, read_len, count, k, queries, n_queries, best_query, best_pos, best_dist, second_query, second_pos, second_dist, err);
}
int bitnuc_reads_hdist_best2_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                    uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                    uint8_t *second_dist, bitnuc_err *err) {
    return reads_best2_packed_host(c, words, read_len, count, k, queries, n_queries, best_query, best_pos, best_dist, second_query, second_pos, second_dist, err);
}
int bitnuc_reads_hdist_anchored_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                      uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_async(c, d_reads, read_len, count, k, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query,
                                d_second_pos, d_second_dist, err);
}
int bitnuc_reads_hdist_anchored_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                             const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                             uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_packed_async(c, d_words, read_len, count, k, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query,
                                       d_second_pos, d_second_dist, err);
}
int bitnuc_reads_hdist_anchored(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const uint64_t *queries,
                                size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_host(c, reads, read_len, count, k, pos_lo, pos_hi, queries, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                               second_dist, err);
}
int bitnuc_reads_hdist_anchored_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                       const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                       uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_packed_host(c, words, read_len, count, k, pos_lo, pos_hi, queries, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                                      second_dist, err);
}
int bitnuc_reads_hdist_anchored_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                            size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos,
                                            uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_batch_async(c, d_seq, d_offsets, count, total_bases, k, anchor, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist,
                                      d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_hdist_anchored_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                   size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries,
                                                   uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                   uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, anchor, pos_lo, pos_hi, d_queries, n_queries, d_best_query,
                                             d_best_pos, d_best_dist, d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_hdist_anchored_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                      uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_batch_host(c, seq, offsets, count, k, anchor, pos_lo, pos_hi, queries, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                                     second_dist, err);
}
int bitnuc_reads_hdist_anchored_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                             int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *queries, size_t n_queries, uint32_t *best_query,
                                             uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_batch_packed_host(c, words, word_offsets, offsets, count, k, anchor, pos_lo, pos_hi, queries, n_queries, best_query, best_pos, best_dist,
                                            second_query, second_pos, second_dist, err);
}
int bitnuc_reads_hdist_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                        const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_batch_async(c, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_hdist_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                               size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query,
                                               uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_hdist_best_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_batch_host(c, seq, offsets, count, k, queries, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_hdist_best_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                         const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_batch_packed_host(c, words, word_offsets, offsets, count, k, queries, n_queries, best_query, best_pos, best_dist, err);
}

// pattern queries: the twins of the twenty above
int bitnuc_reads_pattern_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                    uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_async(c, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_pattern_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                           size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_packed_async(c, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_pattern_best(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                              uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_host(c, reads, read_len, count, k, patterns, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_pattern_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                     uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_packed_host(c, words, read_len, count, k, patterns, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_pattern_best2_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                     uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos,
                                     uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_best2_async(c, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_pattern_best2_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                            size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                            uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_best2_packed_async(c, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos,
                                    d_second_dist, err);
}
int bitnuc_reads_pattern_best2(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                               uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                               bitnuc_err *err) {
    return reads_best2_host(c, reads, read_len, count, k, patterns, n_queries, best_query, best_pos, best_dist, second_query, second_pos, second_dist, err);
}
int bitnuc_reads_pattern_best2_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                      uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                      uint8_t *second_dist, bitnuc_err *err) {
    return reads_best2_packed_host(c, words, read_len, count, k, patterns, n_queries, best_query, best_pos, best_dist, second_query, second_pos, second_dist, err);
}
int bitnuc_reads_pattern_anchored_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                        uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_async(c, d_reads, read_len, count, k, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query,
                                d_second_pos, d_second_dist, err);
}
int bitnuc_reads_pattern_anchored_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                               const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                               uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_packed_async(c, d_words, read_len, count, k, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query,
                                       d_second_pos, d_second_dist, err);
}
int bitnuc_reads_pattern_anchored(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                  const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                  uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_host(c, reads, read_len, count, k, pos_lo, pos_hi, patterns, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                               second_dist, err);
}
int bitnuc_reads_pattern_anchored_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                         const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                         uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_packed_host(c, words, read_len, count, k, pos_lo, pos_hi, patterns, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                                      second_dist, err);
}
int bitnuc_reads_pattern_anchored_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                              size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                              uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist,
                                              bitnuc_err *err) {
    return reads_anchored_batch_async(c, d_seq, d_offsets, count, total_bases, k, anchor, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist,
                                      d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_pattern_anchored_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                     size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns,
                                                     size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                     uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_anchored_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, anchor, pos_lo, pos_hi, d_patterns, n_queries, d_best_query,
                                             d_best_pos, d_best_dist, d_second_query, d_second_pos, d_second_dist, err);
}
int bitnuc_reads_pattern_anchored_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                        uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    return reads_anchored_batch_host(c, seq, offsets, count, k, anchor, pos_lo, pos_hi, patterns, n_queries, best_query, best_pos, best_dist, second_query, second_pos,
                                     second_dist, err);
}
int bitnuc_reads_pattern_anchored_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                               int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query,
                                               uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                                               bitnuc_err *err) {
    return reads_anchored_batch_packed_host(c, words, word_offsets, offsets, count, k, anchor, pos_lo, pos_hi, patterns, n_queries, best_query, best_pos, best_dist,
                                            second_query, second_pos, second_dist, err);
}
int bitnuc_reads_pattern_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                          const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                          bitnuc_err *err) {
    return reads_best_batch_async(c, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_pattern_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                 size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                 uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_best_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, err);
}
int bitnuc_reads_pattern_best_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns,
                                    size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_best_batch_host(c, seq, offsets, count, k, patterns, n_queries, best_query, best_pos, best_dist, err);
}
int bitnuc_reads_pattern_best_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                           const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                           bitnuc_err *err) {
    return reads_best_batch_packed_host(c, words, word_offsets, offsets, count, k, patterns, n_queries, best_query, best_pos, best_dist, err);
}

// the indel-tolerant anchored forms (edit distance): exact queries and their pattern twins
int bitnuc_reads_edist_anchored_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                      uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_async(c, d_reads, read_len, count, k, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                             d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_anchored_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                             const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                             uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_packed_async(c, d_words, read_len, count, k, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                                    d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_anchored(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_host(c, reads, read_len, count, k, pos_lo, pos_hi, queries, n_queries, best_query, best_end, best_dist, second_query,
                            second_end, second_dist, err);
}
int bitnuc_reads_edist_anchored_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                       const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                       uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_packed_host(c, words, read_len, count, k, pos_lo, pos_hi, queries, n_queries, best_query, best_end, best_dist, second_query,
                                   second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                              const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                              uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_async(c, d_reads, read_len, count, k, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                             d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                                     const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                                     uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_packed_async(c, d_words, read_len, count, k, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                                    d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                        uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_host(c, reads, read_len, count, k, pos_lo, pos_hi, patterns, n_queries, best_query, best_end, best_dist, second_query,
                            second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                               const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                               uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_packed_host(c, words, read_len, count, k, pos_lo, pos_hi, patterns, n_queries, best_query, best_end, best_dist, second_query,
                                   second_end, second_dist, err);
}
// the ragged twins
int bitnuc_reads_edist_anchored_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                            size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                            uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_batch_async(c, d_seq, d_offsets, count, total_bases, k, anchor, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_end, d_best_dist,
                                   d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_anchored_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                   size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries,
                                                   uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                                   uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, anchor, pos_lo, pos_hi, d_queries, n_queries, d_best_query, d_best_end,
                                          d_best_dist, d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_anchored_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                      uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_batch_host(c, seq, offsets, count, k, anchor, pos_lo, pos_hi, queries, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist,
                                  err);
}
int bitnuc_reads_edist_anchored_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int anchor,
                                             size_t pos_lo, size_t pos_hi, const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end,
                                             uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_batch_packed_host(c, words, word_offsets, offsets, count, k, anchor, pos_lo, pos_hi, queries, n_queries, best_query, best_end, best_dist, second_query,
                                         second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                                    size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                    uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist,
                                                    bitnuc_err *err) {
    return reads_edist_batch_async(c, d_seq, d_offsets, count, total_bases, k, anchor, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                   d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                           size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns,
                                                           size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                           uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, anchor, pos_lo, pos_hi, d_patterns, n_queries, d_best_query, d_best_end,
                                          d_best_dist, d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                              const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                              uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_batch_host(c, seq, offsets, count, k, anchor, pos_lo, pos_hi, patterns, n_queries, best_query, best_end, best_dist, second_query, second_end,
                                  second_dist, err);
}
int bitnuc_reads_pattern_edist_anchored_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                     int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query,
                                                     uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                                     bitnuc_err *err) {
    return reads_edist_batch_packed_host(c, words, word_offsets, offsets, count, k, anchor, pos_lo, pos_hi, patterns, n_queries, best_query, best_end, best_dist, second_query,
                                         second_end, second_dist, err);
}

// the indel-tolerant best match and runner-up over the whole read (edit distance): fixed, exact queries and their pattern twins; then ragged
int bitnuc_reads_edist_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                  uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                  uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_async(c, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query, d_second_end,
                                  d_second_dist, err);
}
int bitnuc_reads_edist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                         uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                         uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_packed_async(c, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query, d_second_end,
                                         d_second_dist, err);
}
int bitnuc_reads_edist_best(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries, uint32_t *best_query,
                            uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_best_host(c, reads, read_len, count, k, queries, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_edist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                   uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                   bitnuc_err *err) {
    return reads_edist_best_packed_host(c, words, read_len, count, k, queries, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                          size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                          uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_async(c, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query, d_second_end,
                                  d_second_dist, err);
}
int bitnuc_reads_pattern_edist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                                 size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                 uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_packed_async(c, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query, d_second_end,
                                         d_second_dist, err);
}
int bitnuc_reads_pattern_edist_best(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                    uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                    bitnuc_err *err) {
    return reads_edist_best_host(c, reads, read_len, count, k, patterns, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns,
                                           size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                           uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_best_packed_host(c, words, read_len, count, k, patterns, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_edist_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                        const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                        uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_async(c, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                                        d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                               size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                               uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist,
                                               d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_edist_best_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                  bitnuc_err *err) {
    return reads_edist_best_batch_host(c, seq, offsets, count, k, queries, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_edist_best_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                         const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                         uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_packed_host(c, words, word_offsets, offsets, count, k, queries, n_queries, best_query, best_end, best_dist, second_query, second_end,
                                              second_dist, err);
}
int bitnuc_reads_pattern_edist_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                                const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                                uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_async(c, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query,
                                        d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                       size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                       uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                                       uint8_t *d_second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_packed_async(c, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                               d_second_query, d_second_end, d_second_dist, err);
}
int bitnuc_reads_pattern_edist_best_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns,
                                          size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                          uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_host(c, seq, offsets, count, k, patterns, n_queries, best_query, best_end, best_dist, second_query, second_end, second_dist, err);
}
int bitnuc_reads_pattern_edist_best_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                 const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                                 uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    return reads_edist_best_batch_packed_host(c, words, word_offsets, offsets, count, k, patterns, n_queries, best_query, best_end, best_dist, second_query, second_end,
                                              second_dist, err);
}

// ---- pattern queries: a set of bases per position (bitnuc_pattern).  The converters are host code; the twelve entry points behind them are
// the twins of the exact hit lists, counts and best matches above: the same skeleton, input and search under the other query kind.
int bitnuc_pattern_from_iupac(const uint8_t *letters, size_t k, bitnuc_pattern *out, bitnuc_err *err) {
    clear_err(err);
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k); // before any letter is read
    if (!out || (!letters && k)) return fail(err, BITNUC_UNSUPPORTED);
    PatternSets p;
    const long long bad = bitnuc_host::pattern_from_iupac(letters, k, &p);
    if (bad >= 0) return fail_invalid_base(err, letters[bad], (uint64_t)bad);
    memcpy(out, &p, sizeof p);
    return BITNUC_OK;
}

int bitnuc_pattern_from_2bit(uint64_t query, size_t k, bitnuc_pattern *out, bitnuc_err *err) {
    clear_err(err);
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (!out) return fail(err, BITNUC_UNSUPPORTED);
    const PatternSets p = pattern_of_2bit(query, k);
    memcpy(out, &p, sizeof p);
    return BITNUC_OK;
}

int bitnuc_kmer_pattern_count_multi_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, const uint32_t *d_taus, size_t n_queries,
                                          uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistCount<bitnuc_pattern>{d_patterns, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_pattern_count_multi_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                                 const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistCount<bitnuc_pattern>{d_patterns, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_pattern_count_multi(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus, size_t n_queries,
                                    uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistCount<bitnuc_pattern>{patterns, taus, n_queries, counts}, err);
}
int bitnuc_kmer_pattern_count_multi_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus,
                                           size_t n_queries, uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistCount<bitnuc_pattern>{patterns, taus, n_queries, counts}, err);
}
int bitnuc_kmer_pattern_best_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint64_t *d_pos,
                                   uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistBest<bitnuc_pattern>{d_patterns, n_queries, d_pos, d_dist}, err);
}
int bitnuc_kmer_pattern_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                          uint64_t *d_pos, uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistBest<bitnuc_pattern>{d_patterns, n_queries, d_pos, d_dist}, err);
}
int bitnuc_kmer_pattern_best(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *pos, uint8_t *dist,
                             bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistBest<bitnuc_pattern>{patterns, n_queries, pos, dist}, err);
}
int bitnuc_kmer_pattern_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *pos,
                                    uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistBest<bitnuc_pattern>{patterns, n_queries, pos, dist}, err);
}

// ---- the mismatch histogram per query, each form once per query kind
int bitnuc_kmer_hdist_hist_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, size_t n_bins,
                                 uint64_t *d_hist, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistHist<uint64_t>{d_queries, n_queries, n_bins, d_hist}, err);
}
int bitnuc_kmer_hdist_hist_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries,
                                        size_t n_bins, uint64_t *d_hist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistHist<uint64_t>{d_queries, n_queries, n_bins, d_hist}, err);
}
int bitnuc_kmer_hdist_hist(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, size_t n_bins, uint64_t *hist,
                           bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistHist<uint64_t>{queries, n_queries, n_bins, hist}, err);
}
int bitnuc_kmer_hdist_hist_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries, size_t n_bins,
                                  uint64_t *hist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistHist<uint64_t>{queries, n_queries, n_bins, hist}, err);
}
int bitnuc_kmer_pattern_hist_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t n_bins,
                                   uint64_t *d_hist, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistHist<bitnuc_pattern>{d_patterns, n_queries, n_bins, d_hist}, err);
}
int bitnuc_kmer_pattern_hist_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                          size_t n_queries, size_t n_bins, uint64_t *d_hist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistHist<bitnuc_pattern>{d_patterns, n_queries, n_bins, d_hist}, err);
}
int bitnuc_kmer_pattern_hist(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t n_bins, uint64_t *hist,
                             bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistHist<bitnuc_pattern>{patterns, n_queries, n_bins, hist}, err);
}
int bitnuc_kmer_pattern_hist_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                    size_t n_bins, uint64_t *hist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistHist<bitnuc_pattern>{patterns, n_queries, n_bins, hist}, err);
}
int bitnuc_kmer_pattern_hits_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *d_pos, uint8_t *d_hit_dist,
                                   size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, HdistHits<bitnuc_pattern>{pattern, tau, d_pos, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_pattern_hits_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *d_pos,
                                          uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, HdistHits<bitnuc_pattern>{pattern, tau, d_pos, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_pattern_hits(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *pos, uint8_t *hit_dist, size_t cap,
                             uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, HdistHits<bitnuc_pattern>{pattern, tau, pos, hit_dist, cap, n_hits}, err);
}
int bitnuc_kmer_pattern_hits_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *pos,
                                    uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, HdistHits<bitnuc_pattern>{pattern, tau, pos, hit_dist, cap, n_hits}, err);
}

// ---- the indel-tolerant search along a reference: best match and count per query by edit distance, each form once per query kind
int bitnuc_kmer_edist_best_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, uint64_t *d_end, uint8_t *d_dist,
                                 bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistBest<uint64_t>{d_queries, n_queries, d_end, d_dist}, err);
}
int bitnuc_kmer_edist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries,
                                        uint64_t *d_end, uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistBest<uint64_t>{d_queries, n_queries, d_end, d_dist}, err);
}
int bitnuc_kmer_edist_best(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *end, uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistBest<uint64_t>{queries, n_queries, end, dist}, err);
}
int bitnuc_kmer_edist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *end,
                                  uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistBest<uint64_t>{queries, n_queries, end, dist}, err);
}
int bitnuc_kmer_edist_count_multi_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, const uint32_t *d_taus, size_t n_queries,
                                        uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistCount<uint64_t>{d_queries, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_edist_count_multi_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                               const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistCount<uint64_t>{d_queries, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_edist_count_multi(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus, size_t n_queries, uint64_t *counts,
                                  bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistCount<uint64_t>{queries, taus, n_queries, counts}, err);
}
int bitnuc_kmer_edist_count_multi_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus,
                                         size_t n_queries, uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistCount<uint64_t>{queries, taus, n_queries, counts}, err);
}
int bitnuc_kmer_pattern_edist_best_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint64_t *d_end, uint8_t *d_dist,
                                         bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistBest<bitnuc_pattern>{d_patterns, n_queries, d_end, d_dist}, err);
}
int bitnuc_kmer_pattern_edist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                                uint64_t *d_end, uint8_t *d_dist, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistBest<bitnuc_pattern>{d_patterns, n_queries, d_end, d_dist}, err);
}
int bitnuc_kmer_pattern_edist_best(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *end, uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistBest<bitnuc_pattern>{patterns, n_queries, end, dist}, err);
}
int bitnuc_kmer_pattern_edist_best_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *end,
                                          uint8_t *dist, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistBest<bitnuc_pattern>{patterns, n_queries, end, dist}, err);
}
int bitnuc_kmer_pattern_edist_count_multi_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, const uint32_t *d_taus, size_t n_queries,
                                                uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistCount<bitnuc_pattern>{d_patterns, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_pattern_edist_count_multi_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                                       const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistCount<bitnuc_pattern>{d_patterns, d_taus, n_queries, d_counts}, err);
}
int bitnuc_kmer_pattern_edist_count_multi(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus, size_t n_queries, uint64_t *counts,
                                          bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistCount<bitnuc_pattern>{patterns, taus, n_queries, counts}, err);
}
int bitnuc_kmer_pattern_edist_count_multi_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus,
                                                 size_t n_queries, uint64_t *counts, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistCount<bitnuc_pattern>{patterns, taus, n_queries, counts}, err);
}

// ---- the indel-tolerant hit list: the ends within tau along a reference
int bitnuc_kmer_edist_hits_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_end, uint8_t *d_hit_dist, size_t cap,
                                 uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistHits<uint64_t>{&query, tau, d_end, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_edist_hits_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_end,
                                        uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistHits<uint64_t>{&query, tau, d_end, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_edist_hits(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *end, uint8_t *hit_dist, size_t cap, uint64_t *n_hits,
                           bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistHits<uint64_t>{&query, tau, end, hit_dist, cap, n_hits}, err);
}
int bitnuc_kmer_edist_hits_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *end, uint8_t *hit_dist,
                                  size_t cap, uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistHits<uint64_t>{&query, tau, end, hit_dist, cap, n_hits}, err);
}
int bitnuc_kmer_pattern_edist_hits_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *d_end, uint8_t *d_hit_dist,
                                         size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, AsciiRef{d_ref, n}, k, EdistHits<bitnuc_pattern>{pattern, tau, d_end, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_pattern_edist_hits_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau,
                                                uint64_t *d_end, uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err) {
    return ref_async(c, PackedRef{d_words, n_words, n}, k, EdistHits<bitnuc_pattern>{pattern, tau, d_end, d_hit_dist, cap, d_n_hits}, err);
}
int bitnuc_kmer_pattern_edist_hits(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *end, uint8_t *hit_dist, size_t cap,
                                   uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, AsciiRef{ref, n}, k, EdistHits<bitnuc_pattern>{pattern, tau, end, hit_dist, cap, n_hits}, err);
}
int bitnuc_kmer_pattern_edist_hits_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *end,
                                          uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err) {
    return ref_host(c, PackedRef{words, n_words, n}, k, EdistHits<bitnuc_pattern>{pattern, tau, end, hit_dist, cap, n_hits}, err);
}

// ---- the 3' adapter per read: full or overhanging match, with the cut point (reads_dispatch.h) ----
int bitnuc_reads_edist_adapter_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, FixedAscii{d_reads, read_len}, count, AdapterArgs<uint64_t>{k, d_queries, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_edist_adapter_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, FixedPacked{d_words, read_len}, count, AdapterArgs<uint64_t>{k, d_queries, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_edist_adapter_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, AdapterArgs<uint64_t>{k, d_queries, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_edist_adapter_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count, AdapterArgs<uint64_t>{k, d_queries, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_edist_adapter(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, FixedAscii{reads, read_len}, count, AdapterArgs<uint64_t>{k, queries, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_edist_adapter_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, FixedPacked{words, read_len}, count, AdapterArgs<uint64_t>{k, queries, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_edist_adapter_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, RaggedAscii{seq, offsets}, count, AdapterArgs<uint64_t>{k, queries, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_edist_adapter_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, RaggedPacked{words, word_offsets, offsets}, count, AdapterArgs<uint64_t>{k, queries, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, FixedAscii{d_reads, read_len}, count, AdapterArgs<bitnuc_pattern>{k, d_patterns, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, FixedPacked{d_words, read_len}, count, AdapterArgs<bitnuc_pattern>{k, d_patterns, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, AdapterArgs<bitnuc_pattern>{k, d_patterns, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err) {
    return reads_adapter_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count, AdapterArgs<bitnuc_pattern>{k, d_patterns, n_queries, min_overlap, err_num, err_den, {d_adapter, d_cut, d_end, d_overlap, d_dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, FixedAscii{reads, read_len}, count, AdapterArgs<bitnuc_pattern>{k, patterns, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, FixedPacked{words, read_len}, count, AdapterArgs<bitnuc_pattern>{k, patterns, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, RaggedAscii{seq, offsets}, count, AdapterArgs<bitnuc_pattern>{k, patterns, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}
int bitnuc_reads_pattern_edist_adapter_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err) {
    return reads_adapter_host(c, RaggedPacked{words, word_offsets, offsets}, count, AdapterArgs<bitnuc_pattern>{k, patterns, n_queries, min_overlap, err_num, err_den, {adapter, cut, end, overlap, dist}}, err);
}

// ---- the indel-tolerant family's second stage: where the alignment that ends at a given base starts (reads_dispatch.h, ref_dispatch.h) ----
int bitnuc_reads_edist_start_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, FixedAscii{d_reads, read_len}, count, StartArgs<uint64_t>{k, anchor, pos, d_queries, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_edist_start_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, FixedPacked{d_words, read_len}, count, StartArgs<uint64_t>{k, anchor, pos, d_queries, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_edist_start_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor, size_t pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, StartArgs<uint64_t>{k, anchor, pos, d_queries, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_edist_start_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, size_t k, int anchor, size_t pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count, StartArgs<uint64_t>{k, anchor, pos, d_queries, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_edist_start(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, FixedAscii{reads, read_len}, count, StartArgs<uint64_t>{k, anchor, pos, queries, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_edist_start_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, FixedPacked{words, read_len}, count, StartArgs<uint64_t>{k, anchor, pos, queries, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_edist_start_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, RaggedAscii{seq, offsets}, count, StartArgs<uint64_t>{k, anchor, pos, queries, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_edist_start_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, RaggedPacked{words, word_offsets, offsets}, count, StartArgs<uint64_t>{k, anchor, pos, queries, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_pattern_edist_start_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, FixedAscii{d_reads, read_len}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, d_patterns, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_pattern_edist_start_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, FixedPacked{d_words, read_len}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, d_patterns, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_pattern_edist_start_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor, size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, d_patterns, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_pattern_edist_start_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, size_t k, int anchor, size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return reads_start_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count, StartArgs<bitnuc_pattern>{k, anchor, pos, d_patterns, n_queries, d_query, d_end, d_start, d_dist}, err);
}
int bitnuc_reads_pattern_edist_start(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, FixedAscii{reads, read_len}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, patterns, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_pattern_edist_start_packed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, FixedPacked{words, read_len}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, patterns, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_pattern_edist_start_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, RaggedAscii{seq, offsets}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, patterns, n_queries, query, end, start, dist}, err);
}
int bitnuc_reads_pattern_edist_start_batch_packed(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err) {
    return reads_start_host(c, RaggedPacked{words, word_offsets, offsets}, count, StartArgs<bitnuc_pattern>{k, anchor, pos, patterns, n_queries, query, end, start, dist}, err);
}
int bitnuc_ref_edist_start_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return ref_start_async(c, AsciiRef{d_ref, n}, k, RefStartArgs<uint64_t>{d_queries, n_queries, d_query_index, d_end, m, d_m, d_start, d_dist}, err);
}
int bitnuc_ref_edist_start_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return ref_start_async(c, PackedRef{d_words, n_words, n}, k, RefStartArgs<uint64_t>{d_queries, n_queries, d_query_index, d_end, m, d_m, d_start, d_dist}, err);
}
int bitnuc_ref_edist_start(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, const uint32_t *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err) {
    (void)c; // an item reads at most 63 bases: always on the host
    return ref_start_host(AsciiRef{ref, n}, k, RefStartArgs<uint64_t>{queries, n_queries, query_index, end, m, nullptr, start, dist}, err);
}
int bitnuc_ref_edist_start_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries, const uint32_t *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err) {
    (void)c;
    return ref_start_host(PackedRef{words, n_words, n}, k, RefStartArgs<uint64_t>{queries, n_queries, query_index, end, m, nullptr, start, dist}, err);
}
int bitnuc_ref_pattern_edist_start_async(bitnuc_ctx *c, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return ref_start_async(c, AsciiRef{d_ref, n}, k, RefStartArgs<bitnuc_pattern>{d_patterns, n_queries, d_query_index, d_end, m, d_m, d_start, d_dist}, err);
}
int bitnuc_ref_pattern_edist_start_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err) {
    return ref_start_async(c, PackedRef{d_words, n_words, n}, k, RefStartArgs<bitnuc_pattern>{d_patterns, n_queries, d_query_index, d_end, m, d_m, d_start, d_dist}, err);
}
int bitnuc_ref_pattern_edist_start(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err) {
    (void)c; // an item reads at most 63 bases: always on the host
    return ref_start_host(AsciiRef{ref, n}, k, RefStartArgs<bitnuc_pattern>{patterns, n_queries, query_index, end, m, nullptr, start, dist}, err);
}
int bitnuc_ref_pattern_edist_start_packed(bitnuc_ctx *c, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err) {
    (void)c;
    return ref_start_host(PackedRef{words, n_words, n}, k, RefStartArgs<bitnuc_pattern>{patterns, n_queries, query_index, end, m, nullptr, start, dist}, err);
}

} // extern "C"
