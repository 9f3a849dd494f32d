// kmer_launch.h -- the evidence build's dispatch of kmer.hip's launchers: the k-mer batch, the sliding scan, its fused count and
// the bulk hdist in the formulations that lost their A/B (profiles/), selected by the context's SweepKnobs.  Included once, by
// kmer.hip inside its anonymous namespace, under -DBITNUC_SWEEP_VARIANTS.  Host code only; the kernels are in kmer_evidence.h and
// scan_mfma_evidence.h.  wants_<x> is false when every knob it reads holds its shipped value: kmer.hip's own launch code runs then.
#pragma once

namespace evidence {

// ---- launch_batch: which legs a batch uses and their kernels' loads / stores / items per wave / block / rounds per trip ---------------
bool wants_batch(const bitnuc_ctx *c) {
    const SweepKnobs &s = knobs(c);
    return s.batch_dense != 1 || s.batch_slide != 1 || s.slide_impl != 1 || s.dense_policy != kDensePolicy || s.kmer_block != kKmerBlock ||
           s.dense_unroll != kDenseUnroll || s.slide2_rounds != kSlide2Rounds || s.slide_rounds != kSlideRounds;
}

struct KnobLegs { // batch_legs' legs at the context's knobs (slide_impl 0: stride-1 batches take the rounds of 992 windows)
    const SweepKnobs &s;
    bool dense, slide2, slide, nts;
    explicit KnobLegs(const bitnuc_ctx *c)
        : s(knobs(c)), dense(s.batch_dense != 0), slide2(s.batch_slide && s.slide_impl == 1), slide(s.batch_slide != 0), nts((s.dense_policy & 2) != 0) {}
    hipError_t launch_dense(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long items, unsigned long long *o, unsigned long long *slot) const {
        const int kb = s.kmer_block, un = s.dense_unroll;
        if (!aligned16(kmers)) return dense_t<false, false, false, 1>(c, kmers, k, items, o, slot, kb);
#define DENSE(NL, NS) (un == 1 ? dense_t<true, NL, NS, 1>(c, kmers, k, items, o, slot, kb) : un == 2 ? dense_t<true, NL, NS, 2>(c, kmers, k, items, o, slot, kb) \
                                                                                              : dense_t<true, NL, NS, 4>(c, kmers, k, items, o, slot, kb))
        switch (s.dense_policy) { // bit0: nt loads, bit1: nt stores
        case 0: return DENSE(false, false);
        case 1: return DENSE(true, false);
        case 2: return DENSE(false, true);
        default: return DENSE(true, true);
        }
#undef DENSE
    }
    hipError_t launch_slide2(bitnuc_ctx *c, const uint8_t *kmers, size_t k, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) const {
        if (s.slide2_rounds == 1) return nts ? slide2_t<true, 1>(c, kmers, k, rounds, o, slot) : slide2_t<false, 1>(c, kmers, k, rounds, o, slot);
        if (s.slide2_rounds == 2) return nts ? slide2_t<true, 2>(c, kmers, k, rounds, o, slot) : slide2_t<false, 2>(c, kmers, k, rounds, o, slot);
        return nts ? slide2_t<true, 4>(c, kmers, k, rounds, o, slot) : slide2_t<false, 4>(c, kmers, k, rounds, o, slot);
    }
    hipError_t launch_slide(bitnuc_ctx *c, const uint8_t *kmers, size_t k, size_t stride, unsigned long long rounds, unsigned long long *o, unsigned long long *slot) const {
#define SLIDE(P) (nts ? slide_t<true, P>(c, kmers, k, stride, rounds, o, slot) : slide_t<false, P>(c, kmers, k, stride, rounds, o, slot))
        const int p = s.slide_rounds;
        return p == 2 ? SLIDE(2) : p == 4 ? SLIDE(4) : p == 8 ? SLIDE(8) : SLIDE(1);
#undef SLIDE
    }
};

// ---- launch_scan -----------------------------------------------------------------------------------------------------------------
// The query's operand of the natural-layout matrix-core scan (scan_mfma_evidence.h: ScanMfmaTable): per window shift rho and K-step, the nibbles that
// are 1.0 where a channel differs from the query's base (hamming/scalar.rs:33-47 counts the differing 2-bit fields).
// match = true: the nibbles are -1.0 (0b1010) where a channel EQUALS the query's base and the accumulators start at 2^23 + k 2^(8 (r & 3)) (r & 3 = 3: 2^23 + k): the
// product counts the matches down from k -- the same distance with a third of the non-zero entries (one channel of four instead of three).
void scan_mfma_table(uint64_t query, size_t k, ScanMfmaTable *t, bool match = false) {
    uint8_t lo[80], hi[80]; // [16 + i]: channels (A, C) and (G, T) of query position i; zero outside [0, k)
    memset(lo, 0, sizeof lo);
    memset(hi, 0, sizeof hi);
    for (size_t i = 0; i < k; ++i) {
        const unsigned q = (unsigned)((query >> (2 * i)) & 3);
        if (match) {
            lo[16 + i] = (uint8_t)((q == 0 ? 0x0A : 0) | (q == 1 ? 0xA0 : 0));
            hi[16 + i] = (uint8_t)((q == 2 ? 0x0A : 0) | (q == 3 ? 0xA0 : 0));
        } else {
            lo[16 + i] = (uint8_t)((q != 0 ? 0x02 : 0) | (q != 1 ? 0x20 : 0));
            hi[16 + i] = (uint8_t)((q != 2 ? 0x02 : 0) | (q != 3 ? 0x20 : 0));
        }
    }
    for (int j = 0; j < 4; ++j) t->c[j] = kPackBias + (match ? (float)((unsigned)k << (j == 3 ? 0 : 8 * j)) : 0.f);
    memset(t->w[16], 0, sizeof t->w[16]);
    for (int rho = 0; rho < 16; ++rho)
        for (int s = 0; s < 6; ++s)
            for (int i = 0; i < 4; ++i) {
                const int p0 = 16 * (s >> 1) + 8 * (s & 1) + 4 * (i >> 1); // position of byte 0 of this dword
                const uint8_t *src = (i & 1) ? hi : lo;
                uint32_t w = 0;
                for (int b = 0; b < 4; ++b) w |= (uint32_t)src[16 + p0 + b - rho] << (8 * b);
                t->w[rho][4 * s + i] = w;
            }
}

// grid of the natural-layout matrix-core scan: resident waves that walk the rounds (each wave builds its constant operand once)
unsigned scan_mfma_grid(const bitnuc_ctx *c, unsigned long long rounds, int U, bool persist) {
    const unsigned long long want = rounds / ((kBlock / 64) * (unsigned long long)U) + 1; // one trip per wave (+ 1: the tail loop needs a workgroup even without a whole round)
    const unsigned long long cap = persist ? (unsigned long long)c->num_cu * (unsigned)knobs(c).scan_mfma_grid : 0x7FFFFFFFull;
    return (unsigned)(want < cap ? want : cap);
}

// aligned: scan_impl 8 (ships) with workgroups of one wave and trips of four rounds in four channels per base.  Unaligned: the shipped block and unroll.
bool wants_scan(const bitnuc_ctx *c, bool al) {
    const SweepKnobs &s = knobs(c);
    if (!al) return s.kmer_block != kKmerBlock || s.scan_unroll != kScanUnroll;
    return s.scan_impl != 8 || s.scan_mfma_ch3 || s.scan_mfma_block != kScanSegBlock || s.scan_mfma_unroll != kScanSegRounds;
}

hipError_t launch_scan(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist, unsigned long long *slot) {
    const SweepKnobs &s = knobs(c);
    uint32_t ql, qh;
    query_planes(query, k, &ql, &qh);
    const bool al = aligned16(ref) && aligned16(dist);
    const unsigned long long lines = scan_rounds(n); // line-aligned rounds of 1024 windows
    if (s.scan_impl == 8 && al) { // the shipped tiling with three channels per base, workgroups of two or four waves, or other trip lengths
        const int U = s.scan_mfma_unroll;
        if (s.scan_mfma_ch3) { // three channels per base: three MFMAs per 1024 windows
            Count3MfmaTable c3;
            count3_mfma_table(query, k, 0u, &c3, true);
            const unsigned grid = scan_mfma_grid(c, lines, U, false);
            if (U == 2) kmer_scan_seg3_mfma_kernel<3, 2><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, dist, slot, c3);
            else if (U == 3) kmer_scan_seg3_mfma_kernel<3, 3><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, dist, slot, c3);
            else kmer_scan_seg3_mfma_kernel<3, 4><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, dist, slot, c3);
            return hipGetLastError();
        }
        if (s.scan_mfma_block == 128 && U == 4) return scan_seg_t<4, 128>(c, ref, n, k, query, dist, slot); // workgroups of two waves
        return U == 2 ? scan_seg_t<2, kBlock>(c, ref, n, k, query, dist, slot) : U == 3 ? scan_seg_t<3, kBlock>(c, ref, n, k, query, dist, slot)
                      : scan_seg_t<4, kBlock>(c, ref, n, k, query, dist, slot);
    }
    if (s.scan_impl == 7 && al) { // the natural-layout tiling (six MFMAs per 1024 windows, results already in store order): round 5's first matrix-core form
        ScanMfmaTable tab;
        scan_mfma_table(query, k, &tab, s.scan_mfma_match != 0 && s.scan_mfma_pack == 1);
        const int U = s.scan_mfma_unroll, pack = s.scan_mfma_pack, shift = s.scan_mfma_shift;
        const bool persist = s.scan_mfma_persist != 0, ntld = (s.scan_mfma_policy & 1) != 0;
        const unsigned grid = scan_mfma_grid(c, lines, U, persist);
#define SCANM(P, UU, PK, SH, PS) kmer_scan_mfma_kernel<P, UU, false, PK, SH, PS><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, 0u, dist, nullptr, nullptr, nullptr, slot, tab)
#define SCANM_PS(P, UU, PK, SH) do { if (persist) SCANM(P, UU, PK, SH, true); else SCANM(P, UU, PK, SH, false); } while (0)
#define SCANM_NT(UU, PK, SH) do { if (ntld) SCANM_PS(3, UU, PK, SH); else SCANM_PS(2, UU, PK, SH); } while (0)
#define SCANM_U(PK, SH) do { if (U == 2) SCANM_NT(2, PK, SH); else if (U == 3 && SH == 4 && PK == 1) SCANM_NT(3, 1, 4); else SCANM_NT(4, PK, SH); } while (0)
        if (shift == 0) { if (pack == 0) SCANM_PS(3, 2, 0, 0); else SCANM_PS(3, 2, 1, 0); }
        else if (shift == 1) { if (pack == 0) SCANM_U(0, 1); else if (pack == 1) SCANM_U(1, 1); else SCANM_U(2, 1); }
        else if (shift == 2) { if (pack == 0) SCANM_U(0, 2); else if (pack == 1) SCANM_U(1, 2); else SCANM_U(2, 2); }
        else if (shift == 3) { if (pack == 0) SCANM_U(0, 3); else if (pack == 1) SCANM_U(1, 3); else SCANM_U(2, 3); }
        else if (shift == 4) { if (pack == 0) SCANM_U(0, 4); else if (pack == 1) SCANM_U(1, 4); else SCANM_U(2, 4); }
        else if (shift == 6) SCANM_U(1, 6);
        else { if (pack == 0) SCANM_U(0, 5); else SCANM_U(1, 5); }
#undef SCANM_U
#undef SCANM_NT
#undef SCANM_PS
#undef SCANM
        return hipGetLastError();
    }
    const int unroll = s.scan_unroll, kb = s.kmer_block;
    if (s.scan_impl >= 2 && s.scan_impl <= 5 && al) { // line-aligned rounds, a wave owns consecutive rounds and carries the halo planes (kmer_scan3_kernel)
        const int C = s.scan_impl == 2 ? 12 : s.scan_impl == 3 ? 20 : s.scan_impl == 4 ? 16 : 32;
        const unsigned long long waves = (lines + C - 1) / C;
        const unsigned long long blocks = waves / (kBlock / 64) + 1; // (+ 1: the tail loop needs a workgroup even when there is no whole round)
        const unsigned grid = (unsigned)(blocks < 0x7FFFFFFFull ? blocks : 0x7FFFFFFFull);
#define SCAN3(CC) kmer_scan3_kernel<true, true, 4, CC><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, ql, qh, dist, slot)
        if (C == 12) SCAN3(12); else if (C == 20) SCAN3(20); else if (C == 16) SCAN3(16); else SCAN3(32);
#undef SCAN3
        return hipGetLastError();
    }
    // rounds 2-4's bit-plane scan (v_alignbit + v_bcnt per window: VALU-issue bound, profiles/r05_ab_scan_mfma*.txt)
    if (al && s.scan_impl == 1 && unroll == 4 && s.scan_policy == 3 && kb == kBlock) { // GEN 1 (two-LUT planes + scalar halo), what round 4 shipped
        const unsigned grid = grid_for(c, lines / ((kBlock / 64) * 4) + 1, kBlock);
        kmer_scan2_kernel<true, true, true, 4, false, 1><<<grid, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, ql, qh, 0u, dist, nullptr, nullptr, nullptr, slot);
        return hipGetLastError();
    }
    if ((s.scan_impl == 1 || s.scan_impl == 6) && al) { // line-aligned rounds of 1024 windows, round 2-3's plane build (GEN 0; 6 = that form at the shipped policy)
        const unsigned grid = grid_for(c, lines / ((kb / 64) * unroll) + 1, kb);
#define SCAN2(NL, NS, U) kmer_scan2_kernel<true, NL, NS, U, false><<<grid, kb, 0, c->stream>>>(ref, n, (unsigned)k, query, ql, qh, 0u, dist, nullptr, nullptr, nullptr, slot)
#define SCAN2_POLICY(U)                                        \
    switch (s.scan_policy) { /* bit0: nt loads, bit1: nt stores */ \
    case 0: SCAN2(false, false, U); break;                     \
    case 1: SCAN2(true, false, U); break;                      \
    case 2: SCAN2(false, true, U); break;                      \
    default: SCAN2(true, true, U); break;                      \
    }
        if (unroll == 1) { SCAN2_POLICY(1) } else if (unroll == 2) { SCAN2_POLICY(2) } else { SCAN2_POLICY(4) }
#undef SCAN2_POLICY
#undef SCAN2
        return hipGetLastError();
    }
    // scan_impl 0, and unaligned pointers at another block size or unroll: rounds of 992 windows (kmer_scan_kernel)
    if (!al) return scan992_t<false, false, false, 1>(c, ref, n, k, query, dist, slot, kb, unroll);
#define SCAN(NL, NS) (unroll == 1 ? scan992_t<true, NL, NS, 1>(c, ref, n, k, query, dist, slot, kb, unroll) : unroll == 2 ? scan992_t<true, NL, NS, 2>(c, ref, n, k, query, dist, slot, kb, unroll) \
                                                                                                          : scan992_t<true, NL, NS, 4>(c, ref, n, k, query, dist, slot, kb, unroll))
    switch (s.scan_policy) { // bit0: nt loads, bit1: nt stores
    case 0: return SCAN(false, false);
    case 1: return SCAN(true, false);
    case 2: return SCAN(false, true);
    default: return SCAN(true, true);
    }
#undef SCAN
}

// ---- launch_count ----------------------------------------------------------------------------------------------------------------
// aligned: a matrix-core scan_impl (7 or 8) and the shipped three-channel count.  Unaligned: no alternatives.
bool wants_count(const bitnuc_ctx *c, bool al) {
    const SweepKnobs &s = knobs(c);
    return al && (s.scan_impl < 7 || s.scan_mfma_count_form != 2 || s.scan_mfma_count_rounds != kCountRounds || s.scan_mfma_count_grid != kCountGrid);
}

hipError_t launch_count(bitnuc_ctx *c, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, unsigned long long *res,
                        unsigned long long *slot) {
    const SweepKnobs &s = knobs(c);
    const unsigned long long rounds = scan_rounds(n);
    if (s.scan_impl < 7) return count_scan2_t<true, true, 4, 1>(c, ref, n, k, query, tau, res, slot); // round 4's fused count on the bit-plane scan (0.33 ms per 10^9 windows against the matrix-core form's 0.20)
    const int CU_ = s.scan_mfma_count_rounds;
    if (s.scan_mfma_count_form == 2) { // three channels per base at other trip lengths or grids
        const int g = s.scan_mfma_count_grid;
        return CU_ == 2 ? count3_t<2>(c, ref, n, k, query, tau, res, slot, g) : CU_ == 3 ? count3_t<3>(c, ref, n, k, query, tau, res, slot, g) : count3_t<4>(c, ref, n, k, query, tau, res, slot, g);
    }
    if (s.scan_mfma_count_form == 1) { // the count's own tiling: segments of 32 windows, 4 MFMAs per 1024 windows
        CountMfmaTable ct;
        const int emit = s.scan_mfma_count_emit;
        count_mfma_table(query, k, &ct, emit != 0, tau, s.scan_mfma_match != 0);
        const unsigned long long want = rounds / ((kBlock / 64) * (unsigned long long)CU_) + 1, cap = (unsigned long long)c->num_cu * (unsigned)s.scan_mfma_count_grid;
        const unsigned g = (unsigned)(want < cap ? want : cap);
#define COUNTOWN(UU, EM) kmer_count_mfma_kernel<UU, true, EM><<<g, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, tau, res, c->d_acc + 5, c->d_tickets + 2, slot, ct)
#define COUNTOWN_E(UU) do { if (emit == 0) COUNTOWN(UU, 0); else if (emit == 1) COUNTOWN(UU, 1); else COUNTOWN(UU, 2); } while (0)
        if (CU_ == 2) COUNTOWN_E(2); else if (CU_ == 3) COUNTOWN_E(3); else COUNTOWN_E(4);
#undef COUNTOWN_E
#undef COUNTOWN
        return hipGetLastError();
    }
    // the scan's natural-layout tiling (6 MFMAs per 1024 windows)
    ScanMfmaTable tab;
    scan_mfma_table(query, k, &tab);
    const int U = s.scan_mfma_unroll, shift = s.scan_mfma_shift;
    const bool persist = s.scan_mfma_count_persist != 0; // 0: one trip per wave, every workgroup arrives at the ticket (two atomics per workgroup)
    const unsigned g = scan_mfma_grid(c, rounds, U, persist);
    const bool nt = (s.scan_mfma_policy & 1) != 0;
    static_assert(kScanPartials == 1024, "runtime.hip allocates 1024 partial accumulators behind d_acc[8]");
#define COUNTM(P, UU, SH, PS) kmer_scan_mfma_kernel<P, UU, true, 0, SH, PS><<<g, kBlock, 0, c->stream>>>(ref, n, (unsigned)k, query, tau, nullptr, res, PS ? c->d_acc + 5 : c->d_acc + 8, c->d_tickets + 2, slot, tab)
#define COUNTM_PS(P, UU, SH) do { if (persist) COUNTM(P, UU, SH, true); else COUNTM(P, UU, SH, false); } while (0)
#define COUNTM_NT(UU, SH) do { if (nt) COUNTM_PS(1, UU, SH); else COUNTM_PS(0, UU, SH); } while (0)
#define COUNTM_U(SH) do { if (U == 2) COUNTM_NT(2, SH); else COUNTM_NT(4, SH); } while (0)
    if (shift == 0) COUNTM(1, 2, 0, true); else if (shift == 1) COUNTM_U(1); else if (shift == 2) COUNTM_U(2); else if (shift == 3) COUNTM_U(3); else if (shift == 4) COUNTM_U(4); else COUNTM_U(5);
    if (!persist && shift != 0) scan_count_finish_kernel<<<1, kScanPartials, 0, c->stream>>>(c->d_acc + 8, res);
#undef COUNTM_U
#undef COUNTM_NT
#undef COUNTM_PS
#undef COUNTM
    return hipGetLastError();
}

// ---- bitnuc_hdist_dev: grid-stride at tile granularity (16 KiB of each operand per workgroup trip) -------------------------------
bool wants_hdist(const bitnuc_ctx *c) { return knobs(c).hdist_tiled != 0; }

int launch_hdist(bitnuc_ctx *c, unsigned grid, const unsigned long long *a, const unsigned long long *b, size_t n_bases, uint32_t *d_result, bitnuc_err *err) {
    hdist_kernel<true><<<grid, kBlock, 0, c->stream>>>(a, b, n_bases, d_result, reinterpret_cast<unsigned *>(c->d_acc + 4), c->d_tickets + 1);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

} // namespace evidence
