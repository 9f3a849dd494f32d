// codec_launch.h -- the evidence build's dispatch of codec.hip's bulk encode / decode: the 43 variants of encode_kernel /
// decode_kernel that are not shipped, the 16-byte-store encode (encode_quad_kernel), the 8-byte-load decode (decode_x2_kernel), the
// lane-per-base ballot encode and the unused dynamic LDS of the occupancy A/B (dyn_lds).  Included once, by codec.hip inside its
// anonymous namespace, under -DBITNUC_SWEEP_VARIANTS.  Host code only; the kernels are in codec_evidence.h.
#pragma once

namespace evidence {

// the variants that are not shipped (codec.hip's BITNUC_VARIANTS holds the shipped four)
//              id  UNROLL BLOCK NTLD   NTST   XPOSE  XCD
#define BITNUC_EVIDENCE_VARIANTS(X)                   \
    X(1, 4, 256, true, true, false, false)            \
    X(2, 2, 256, true, true, false, false)            \
    X(4, 2, 256, false, false, false, false)          \
    X(5, 4, 256, true, false, false, false)           \
    X(6, 1, 256, true, false, false, false)           \
    X(7, 2, 512, true, false, false, false)           \
    X(8, 2, 1024, true, false, false, false)          \
    X(9, 4, 256, false, false, true, false)           \
    X(10, 4, 256, true, true, true, false)            \
    X(11, 4, 256, true, false, true, false)           \
    X(12, 2, 256, true, false, false, true)           \
    X(13, 4, 256, false, false, false, true)          \
    X(14, 2, 128, true, false, false, false)          \
    X(15, 8, 256, true, false, false, false)          \
    X(16, 4, 512, false, false, false, false)         \
    X(17, 2, 512, false, false, false, false)         \
    X(18, 4, 256, false, true, false, false)          \
    X(19, 4, 512, true, false, true, false)           \
    X(20, 1, 256, false, false, false, false)         \
    X(21, 1, 512, true, false, false, false)          \
    X(23, 4, 1024, false, false, false, false)        \
    X(24, 2, 256, false, false, false, true)          \
    X(25, 4, 256, true, false, false, true)           \
    X(26, 8, 256, false, false, false, true)          \
    X(27, 4, 512, false, false, false, true)          \
    X(28, 4, 256, false, false, true, true)           \
    X(29, 1, 256, false, false, false, true)          \
    X(30, 2, 256, true, true, false, true)            \
    X(31, 4, 256, true, true, false, true)            \
    X(32, 8, 256, true, true, false, false)           \
    X(33, 4, 512, true, true, false, false)           \
    X(34, 4, 256, false, true, false, true)           \
    X(35, 4, 128, true, true, false, false)           \
    X(36, 2, 64, true, false, false, false)           \
    X(37, 4, 128, true, false, false, false)          \
    X(38, 1, 128, true, false, false, false)          \
    X(40, 4, 128, true, true, false, true)            \
    X(41, 2, 512, true, true, false, true)            \
    X(42, 1, 256, true, true, false, true)            \
    X(43, 2, 128, true, false, false, true)           \
    X(44, 1, 128, true, true, false, true)            \
    X(45, 1, 512, true, true, false, true)            \
    X(46, 1, 1024, true, true, false, true)
constexpr int kQuadFirst = 47, kQuadLast = 62; // encode variants of encode_quad_kernel
constexpr int kX2First = 47, kX2Last = 54;     // decode variants of decode_x2_kernel

constexpr int evidence_row(int id) { // -1: not one of these rows; else 1 for the LDS-transpose variants (16-byte aligned buffers on both sides)
    switch (id) {
#define X(vid, U, B, NL, NS, XP, XC) case vid: return XP ? 1 : 0;
        BITNUC_EVIDENCE_VARIANTS(X)
#undef X
    default: return -1;
    }
}
bool encode_variant(int id) { return evidence_row(id) >= 0 || (id >= kQuadFirst && id <= kQuadLast); }
bool decode_variant(int id) { return evidence_row(id) >= 0 || (id >= kX2First && id <= kX2Last); }

// encode variants 47..62: encode_quad_kernel (16-byte stores by a register quad transpose, 4 rounds per wave).
// id - 47: bit 0 = nt loads, bit 1 = nt stores, bit 2 = XCD-contiguous tile order, bit 3 = 256 (not 128) threads per workgroup.
template <int BLOCK>
hipError_t launch_encode_quad_t(bitnuc_ctx *c, int mode, const uint8_t *seq, uint32_t *out32, unsigned long long len, unsigned long long *slot) {
    const unsigned grid = grid_for(c, (len >> 4) / ((unsigned long long)BLOCK * 4) + 1, BLOCK);
#define QUAD(NL, NS, XC) encode_quad_kernel<BLOCK, NL, NS, XC><<<grid, BLOCK, 0, c->stream>>>(seq, out32, len, slot)
    switch (mode & 7) {
    case 0: QUAD(false, false, false); break;
    case 1: QUAD(true, false, false); break;
    case 2: QUAD(false, true, false); break;
    case 3: QUAD(true, true, false); break;
    case 4: QUAD(false, false, true); break;
    case 5: QUAD(true, false, true); break;
    case 6: QUAD(false, true, true); break;
    default: QUAD(true, true, true); break;
    }
#undef QUAD
    return hipGetLastError();
}

bool wants_encode(const bitnuc_ctx *c) { return !shipped_variant(c->enc_variant) || knobs(c).dyn_lds != 0; }

hipError_t launch_encode(bitnuc_ctx *c, const uint8_t *seq, uint64_t *out, unsigned long long len, unsigned long long *slot) {
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    const bool in_al = aligned16(seq), out_al = aligned16(out);
    if (c->enc_variant >= kQuadFirst && c->enc_variant <= kQuadLast && in_al && out_al) {
        const int mode = c->enc_variant - kQuadFirst;
        return (mode & 8) ? launch_encode_quad_t<256>(c, mode, seq, o, len, slot) : launch_encode_quad_t<128>(c, mode, seq, o, len, slot);
    }
    if (c->enc_variant == kBallotVariant) { // lane-per-base + ballot formulation
        const unsigned grid = grid_for(c, ((len + 63) / 64 + (kBlock / 64) * 4 - 1) / ((kBlock / 64) * 4));
        encode_ballot_kernel<4><<<grid, kBlock, 0, c->stream>>>(seq, reinterpret_cast<unsigned long long *>(out), len, slot);
        return hipGetLastError();
    }
    int v = c->enc_variant;
    if (v >= kQuadFirst) v = kDefaultEnc; // a quad variant asked for unaligned buffers: the default kernel handles any alignment
    if (evidence_row(v) == 1 && !(in_al && out_al)) v = kDefaultEnc;
    switch (v) {
#define X(id, U, B, NL, NS, XP, XC) \
    case id: return launch_encode_t<U, B, NL, NS, XP, XC>(c, seq, o, len, slot, XP ? true : in_al, knobs(c).dyn_lds);
        BITNUC_EVIDENCE_VARIANTS(X)
#undef X
    default: return encode_shipped(c, v, seq, o, len, slot, knobs(c).dyn_lds);
    }
}

// decode variants 47..54: decode_x2_kernel (8-byte loads + LDS transpose) for the whole 2 KiB wave tiles, the default
// decode_kernel for what is left.  id - 47: bit 0 = nt loads, bit 1 = plain (not nt) stores, bit 2 = 2 words in flight per lane.
template <int UNROLL>
hipError_t launch_decode_x2_t(bitnuc_ctx *c, int mode, const unsigned long long *w, uint8_t *out, unsigned long long tiles) {
    constexpr int B = 256;
    const unsigned long long per = (unsigned long long)(B / 64) * UNROLL;
    const unsigned grid = (unsigned)((tiles + per - 1) / per);
    switch (mode & 3) {
    case 0: decode_x2_kernel<B, UNROLL, false, true><<<grid, B, 0, c->stream>>>(w, out, tiles); break;
    case 1: decode_x2_kernel<B, UNROLL, true, true><<<grid, B, 0, c->stream>>>(w, out, tiles); break;
    case 2: decode_x2_kernel<B, UNROLL, false, false><<<grid, B, 0, c->stream>>>(w, out, tiles); break;
    default: decode_x2_kernel<B, UNROLL, true, false><<<grid, B, 0, c->stream>>>(w, out, tiles); break;
    }
    return hipGetLastError();
}

bool wants_decode(const bitnuc_ctx *c) { return !shipped_variant(c->dec_variant) || knobs(c).dyn_lds != 0; }

hipError_t launch_decode(bitnuc_ctx *c, const uint64_t *ebuf, uint8_t *out, unsigned long long n_bases) {
    const bool in_al = aligned16(ebuf), out_al = aligned16(out);
    const int lds = knobs(c).dyn_lds;
    if (c->dec_variant >= kX2First && c->dec_variant <= kX2Last && out_al) {
        const unsigned long long tiles = n_bases >> 11; // whole 2 KiB (64-word) wave tiles
        if (tiles) {
            const int mode = c->dec_variant - kX2First;
            const unsigned long long *w = reinterpret_cast<const unsigned long long *>(ebuf);
            const hipError_t rc = (mode & 4) ? launch_decode_x2_t<2>(c, mode, w, out, tiles) : launch_decode_x2_t<1>(c, mode, w, out, tiles);
            if (rc != hipSuccess) return rc;
        }
        const unsigned long long done = tiles << 11;
        if (done == n_bases) return hipSuccess;
        return decode_shipped(c, kDefaultDec, reinterpret_cast<const uint32_t *>(ebuf) + (done >> 4), out + done, n_bases - done, lds); // the rest: the default kernel
    }
    const uint32_t *i = reinterpret_cast<const uint32_t *>(ebuf);
    int v = c->dec_variant;
    if (v >= kX2First) v = kDefaultDec; // x2 asked for an unaligned output: the default kernel handles any alignment
    if (evidence_row(v) == 1 && !in_al) v = kDefaultDec;
    switch (v) {
#define X(id, U, B, NL, NS, XP, XC) \
    case id: return launch_decode_t<U, B, NL, NS, XP, XC>(c, i, out, n_bases, out_al, lds);
        BITNUC_EVIDENCE_VARIANTS(X)
#undef X
    default: return decode_shipped(c, v, i, out, n_bases, lds);
    }
}

// bitnuc_stream_probe_dev mode 5: the every-window kernel's shape: `bytes` of ASCII-side input, 8 x as many bytes written.  bit 4: nt stores,
// bit 5: interleaved map, bits 6-7: rounds per trip 1 / 2 / 4
int probe_window_shape(bitnuc_ctx *c, int mode, const void *d_src, void *d_dst, size_t bytes, bitnuc_err *err) {
    if (!d_src || !d_dst || !aligned16(d_src) || !aligned16(d_dst)) return fail(err, BITNUC_UNSUPPORTED);
    const bool nts = (mode & 16) != 0;
    const u32x4 *src = static_cast<const u32x4 *>(d_src);
    u32x4 *dst = static_cast<u32x4 *>(d_dst);
    const unsigned long long rounds = (bytes >> 10) & ~3ull;
    const int U = 1 << ((mode >> 6) & 3);
    const unsigned g5 = grid_for(c, (rounds + (unsigned long long)U * 4 - 1) / ((unsigned long long)U * 4));
#define WIN(NS, UU, MP) probe_win_shape_kernel<NS, UU, MP><<<g5, kBlock, 0, c->stream>>>(src, dst, rounds)
#define WIN_U(NS, MP) do { if (U == 1) WIN(NS, 1, MP); else if (U == 2) WIN(NS, 2, MP); else WIN(NS, 4, MP); } while (0)
    if (mode & 32) { if (nts) WIN_U(true, 1); else WIN_U(false, 1); }
    else { if (nts) WIN_U(true, 0); else WIN_U(false, 0); }
#undef WIN_U
#undef WIN
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

} // namespace evidence
