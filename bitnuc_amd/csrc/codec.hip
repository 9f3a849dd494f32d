// codec.hip -- bulk 2-bit encode / decode behind the C ABI (include/bitnuc_hip.h): the device-pointer entry points (the
// roofline path), the host-pointer calls with their size dispatch and the pipelined staging of large pageable buffers, the
// single-word API (host code, host_word.h), the synthetic generator and the streaming probes.  Kernels: codec_device.h.
// Reference: encode -> src/utils/mod.rs:22-25 -> packing/avx.rs:130-151; decode -> src/utils/mod.rs:60-62 ->
// unpacking/avx.rs:116-153; as_2bit / from_2bit -> packing/mod.rs:80-110, unpacking/mod.rs:119-147.
#include "runtime.h"
#include "codec_device.h"
#include "host_pipe.h"
#include "host_word.h"

#include <time.h>

using namespace bitnuc_dev;
using namespace bitnuc_rt;

namespace {

// ---- kernel-variant tables -------------------------------------------------------
// The product library ships the variants that are in use: the tuned defaults (encode 39, decode 22), the plain
// reference shape (0) and an earlier default (3).  The other 43, the 16-byte-store and LDS-transpose forms and the
// lane-per-base ballot formulation are measurement evidence (profiles/): evidence/codec_launch.h, compiled only into the
// evidence build, libbitnuc_hip_sweep.so, which tools/sweep*.py and the all-variants parity test load.
//              id  UNROLL BLOCK NTLD   NTST   XPOSE  XCD
#define BITNUC_VARIANTS(X)                            \
    X(0, 4, 256, false, false, false, false)          \
    X(3, 2, 256, true, false, false, false)           \
    X(22, 2, 256, false, true, false, false)          \
    X(39, 2, 128, true, true, false, true)
constexpr int kNumVariants = 47;    // ids 0..46; which of them this build holds: codec_variant_built
constexpr int kBallotVariant = 100; // encode only: lane-per-base + ballot (evidence build; set_variant("encode", 100))
// defaults from the sustained (back-to-back) pair sweeps in profiles/ (10^9 bases, one tile per
// workgroup, interleaved rounds in one process, decode reading words written two steps
// earlier so that none of its input is Infinity-Cache resident -- what bench.py times):
//   encode 39: nt loads + nt stores, 2 groups in flight per lane, 128-thread workgroups, XCD-contiguous tile order
//   decode 22: plain loads + nt stores, 2 groups per lane
// The pair is tuned, not each kernel, and every good pair lands on the same plateau of ~0.40 ms per step = 6.3 TB/s of
// mixed read/write HBM traffic (all 47 x 47 pairs: profiles/r02_sweep_pairs_all_cold.txt; the ten best are within 0.6 %).
// What differs is how the step divides: with encode 14 (plain, allocating stores -- the round-1 default) the 250 MB of
// packed words sit dirty in the 256 MiB Infinity Cache and are written back while the DECODE runs: encode 0.182 ms, decode
// 0.214 ms.  With nt stores the encode pays for its own writes: 0.199-0.204 / 0.194 ms; the step is the same (five processes each:
// 0.4019 vs 0.4024 ms, profiles/r02_encode_variant_stability.txt): a choice of attribution, not of speed.
static_assert(kDefaultEnc == 39 && kDefaultDec == 22, "runtime.h holds the defaults the context starts with");

// lds: bytes of unused dynamic LDS that only limit how many workgroups a CU holds (the evidence build's dyn_lds, tools/ab_occupancy.py)
template <int UNROLL, int BLOCK, bool NTLD, bool NTST, bool XPOSE, bool XCD>
hipError_t launch_encode_t(bitnuc_ctx *c, const uint8_t *seq, uint32_t *out32, unsigned long long len,
                           unsigned long long *slot, bool al, int lds = 0) {
    const unsigned long long tile = (unsigned long long)BLOCK * UNROLL;
    const unsigned grid = grid_for(c, (len >> 4) / tile + 1, BLOCK);
    if (al) encode_kernel<UNROLL, BLOCK, NTLD, NTST, true, XPOSE, XCD><<<grid, BLOCK, lds, c->stream>>>(seq, out32, len, slot);
    else if constexpr (!XPOSE) encode_kernel<UNROLL, BLOCK, NTLD, NTST, false, false, XCD><<<grid, BLOCK, lds, c->stream>>>(seq, out32, len, slot);
    return hipGetLastError();
}

template <int UNROLL, int BLOCK, bool NTLD, bool NTST, bool XPOSE, bool XCD>
hipError_t launch_decode_t(bitnuc_ctx *c, const uint32_t *in32, uint8_t *out, unsigned long long n_bases, bool al, int lds = 0) {
    const unsigned long long tile = (unsigned long long)BLOCK * UNROLL;
    const unsigned grid = grid_for(c, (n_bases >> 4) / tile + 1, BLOCK);
    if (al) decode_kernel<UNROLL, BLOCK, NTLD, NTST, true, XPOSE, XCD><<<grid, BLOCK, lds, c->stream>>>(in32, out, n_bases);
    else decode_kernel<UNROLL, BLOCK, NTLD, NTST, false, XPOSE, XCD><<<grid, BLOCK, lds, c->stream>>>(in32, out, n_bases);
    return hipGetLastError();
}

constexpr bool shipped_variant(int id) {
    switch (id) {
#define X(vid, U, B, NL, NS, XP, XC) case vid: return true;
        BITNUC_VARIANTS(X)
#undef X
    default: return false;
    }
}

// the shipped variant v (the evidence build: with `lds`)
hipError_t encode_shipped(bitnuc_ctx *c, int v, const uint8_t *seq, uint32_t *o, unsigned long long len, unsigned long long *slot, int lds = 0) {
    switch (v) {
#define X(id, U, B, NL, NS, XP, XC) \
    case id: static_assert(!XP, "a shipped LDS-transpose variant needs the aligned-buffer fallback"); return launch_encode_t<U, B, NL, NS, XP, XC>(c, seq, o, len, slot, aligned16(seq), lds);
        BITNUC_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

hipError_t decode_shipped(bitnuc_ctx *c, int v, const uint32_t *i, uint8_t *out, unsigned long long n_bases, int lds = 0) {
    switch (v) {
#define X(id, U, B, NL, NS, XP, XC) \
    case id: static_assert(!XP, "a shipped LDS-transpose variant needs the aligned-buffer fallback"); return launch_decode_t<U, B, NL, NS, XP, XC>(c, i, out, n_bases, aligned16(out), lds);
        BITNUC_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

#ifdef BITNUC_SWEEP_VARIANTS
#include "evidence/codec_launch.h" // the variants that lost their A/B: the hooks below
#endif

hipError_t launch_encode(bitnuc_ctx *c, const uint8_t *seq, uint64_t *out, unsigned long long len, unsigned long long *slot) {
    BITNUC_EVIDENCE(if (evidence::wants_encode(c)) return evidence::launch_encode(c, seq, out, len, slot);)
    return encode_shipped(c, c->enc_variant, seq, reinterpret_cast<uint32_t *>(out), len, slot);
}

hipError_t launch_decode(bitnuc_ctx *c, const uint64_t *ebuf, uint8_t *out, unsigned long long n_bases) {
    BITNUC_EVIDENCE(if (evidence::wants_decode(c)) return evidence::launch_decode(c, ebuf, out, n_bases);)
    return decode_shipped(c, c->dec_variant, reinterpret_cast<const uint32_t *>(ebuf), out, n_bases);
}
} // namespace

namespace bitnuc_rt {
bool codec_variant_built(int id) { return shipped_variant(id) BITNUC_EVIDENCE(|| evidence::encode_variant(id)); }
bool codec_decode_variant_ok(int id) { return shipped_variant(id) BITNUC_EVIDENCE(|| evidence::decode_variant(id)); }
int codec_num_variants() { return kNumVariants; }
int codec_ballot_variant() { return kEvidenceBuild ? kBallotVariant : -1; }
} // namespace bitnuc_rt

// ---- host-pointer jobs: host_pipe.h ---------------------------------------------------------------
namespace {

// items are bases; the pipe's chunks are a multiple of 32 bases, the scratch loop's too (or the whole input)
struct EncodeJob {
    bitnuc_ctx *c; const uint8_t *seq; uint64_t *out; size_t count;
    static constexpr int in_kind = kBufA, out_kind = kBufB;
    static constexpr bool drains = true, inout = false;
    size_t pipe_per(size_t chunk) const { return chunk; }
    size_t scratch_per() const { return kHostChunk; }
    const void *in_src(size_t i0) const { return seq + i0; }
    size_t in_bytes(size_t m) const { return m; }
    void *out_dst(size_t i0) const { return out + i0 / 32; }
    size_t out_bytes(size_t m) const { return words_for(m) * 8; }
    int launch(size_t i0, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err) const {
        unsigned long long *slot;
        if (int st = take_slot(c, i0, &slot, err)) return st;
        HIPCHK(launch_encode(c, d_in, reinterpret_cast<uint64_t *>(d_out), m, slot));
        return BITNUC_OK;
    }
};

struct DecodeJob {
    bitnuc_ctx *c; const uint64_t *ebuf; uint8_t *out; size_t count;
    static constexpr int in_kind = kBufB, out_kind = kBufA;
    static constexpr bool drains = false, inout = false;
    size_t pipe_per(size_t chunk) const { return chunk; }
    size_t scratch_per() const { return kHostChunk; }
    const void *in_src(size_t i0) const { return ebuf + i0 / 32; }
    size_t in_bytes(size_t m) const { return words_for(m) * 8; }
    void *out_dst(size_t i0) const { return out + i0; }
    size_t out_bytes(size_t m) const { return m; }
    int launch(size_t, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err) const {
        HIPCHK(launch_decode(c, reinterpret_cast<const uint64_t *>(d_in), d_out, m));
        return BITNUC_OK;
    }
};

} // namespace

namespace bitnuc_rt {

void pipe_destroy(HostPipe *p) { pipe_free(p); }

int encode_dev_at(bitnuc_ctx *c, const uint8_t *d_seq, size_t len, uint64_t *d_out, unsigned long long index_base, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (len == 0) return BITNUC_OK; // 0 words (the reference panics: packing/avx.rs:138)
    if (!d_seq || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    unsigned long long *slot;
    if (int st = take_slot(c, index_base, &slot, err)) return st;
    HIPCHK(launch_encode(c, d_seq, d_out, len, slot));
    return BITNUC_OK;
}

} // namespace bitnuc_rt

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" {

// Diagnostic (bench.py's host_path block): how the pipelined host-pointer path of this context is configured.  Creates the pipe if
// this context has none yet.  out[0..n): chunk_bases, depth; 0 past them.
int bitnuc_host_pipe_info(bitnuc_ctx *c, double *out, int n, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (!out || n < 1) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    HostPipe *p;
    if (int st = pipe_get(c, &p, err)) return st;
    const double v[2] = {(double)p->chunk, (double)kPipeDepth};
    for (int i = 0; i < n; ++i) out[i] = i < 2 ? v[i] : 0.0;
    return BITNUC_OK;
}

int bitnuc_encode_dev(bitnuc_ctx *c, const uint8_t *d_seq, size_t len, uint64_t *d_out, bitnuc_err *err) {
    return encode_dev_at(c, d_seq, len, d_out, 0, err);
}

int bitnuc_decode_dev(bitnuc_ctx *c, const uint64_t *d_ebuf, size_t n_words, size_t n_bases, uint8_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    // unpacking/mod.rs:40-45: missing words -> InvalidLength(n_bases)
    if (n_words < words_for(n_bases)) return fail(err, BITNUC_INVALID_LENGTH, n_bases);
    if (n_bases == 0) return BITNUC_OK; // unpacking/avx.rs:134-145: nothing appended
    if (!d_ebuf || !d_out || (reinterpret_cast<uintptr_t>(d_ebuf) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    HIPCHK(launch_decode(c, d_ebuf, d_out, n_bases));
    return BITNUC_OK;
}
int bitnuc_nucgen_dev(bitnuc_ctx *c, uint8_t *d_out, size_t len, uint64_t seed, uint64_t first, int flags, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (len == 0) return BITNUC_OK;
    if (!d_out) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    const unsigned grid = grid_for(c, ((len + 15) / 16 + kBlock - 1) / kBlock);
    nucgen_kernel<<<grid, kBlock, 0, c->stream>>>(d_out, len, seed, first, flags);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

int bitnuc_stream_probe_dev(bitnuc_ctx *c, int mode, const void *d_src, void *d_dst, size_t bytes, bitnuc_err *err) {
    // mode: bits 0-2 = 0 read / 1 copy / 2 fill; bit 3 = nt loads; bit 4 = nt stores; bit 5 = 2 (not 4) groups per lane
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    BITNUC_EVIDENCE(if ((mode & 7) == 5) return evidence::probe_window_shape(c, mode, d_src, d_dst, bytes, err);)
    const unsigned long long n16 = bytes / 16;
    const bool ntl = (mode & 8) != 0, nts = (mode & 16) != 0, u2 = (mode & 32) != 0;
    const unsigned grid = grid_for(c, n16 / (kBlock * (u2 ? 2 : 4)) + 1);
    const u32x4 *src = static_cast<const u32x4 *>(d_src);
    u32x4 *dst = static_cast<u32x4 *>(d_dst);
#define PROBE(K, ...) K<<<grid, kBlock, 0, c->stream>>>(__VA_ARGS__)
    switch (mode & 7) {
    case 0:
        if (!d_src || !aligned16(d_src)) return fail(err, BITNUC_UNSUPPORTED);
        if (u2) { if (ntl) PROBE((probe_read_kernel<2, true>), src, n16, c->d_sink); else PROBE((probe_read_kernel<2, false>), src, n16, c->d_sink); }
        else { if (ntl) PROBE((probe_read_kernel<4, true>), src, n16, c->d_sink); else PROBE((probe_read_kernel<4, false>), src, n16, c->d_sink); }
        break;
    case 1:
        if (!d_src || !d_dst || !aligned16(d_src) || !aligned16(d_dst)) return fail(err, BITNUC_UNSUPPORTED);
        if (ntl && nts) PROBE((probe_copy_kernel<4, true, true>), src, dst, n16);
        else if (ntl) PROBE((probe_copy_kernel<4, true, false>), src, dst, n16);
        else if (nts) PROBE((probe_copy_kernel<4, false, true>), src, dst, n16);
        else PROBE((probe_copy_kernel<4, false, false>), src, dst, n16);
        break;
    case 2:
        if (!d_dst || !aligned16(d_dst)) return fail(err, BITNUC_UNSUPPORTED);
        if (nts) PROBE((probe_fill_kernel<4, true>), dst, n16); else PROBE((probe_fill_kernel<4, false>), dst, n16);
        break;
    case 3: { // encode_kernel's shape (variant 39: 2 rounds, 128 threads, nt loads, nt stores, XCD-contiguous tiles): `bytes` of ASCII-side input
        if (!d_src || !d_dst || !aligned16(d_src) || !aligned16(d_dst)) return fail(err, BITNUC_UNSUPPORTED);
        const unsigned g3 = grid_for(c, n16 / (128 * 2) + 1, 128);
        probe_enc_shape_kernel<2, 128, true, true, true><<<g3, 128, 0, c->stream>>>(src, static_cast<uint32_t *>(d_dst), n16);
        break;
    }
    case 4: { // decode_kernel's shape (variant 22: 2 rounds, 256 threads, plain loads, nt stores): `bytes` of ASCII-side output
        if (!d_src || !d_dst || !aligned16(d_src) || !aligned16(d_dst)) return fail(err, BITNUC_UNSUPPORTED);
        const unsigned g4 = grid_for(c, n16 / (256 * 2) + 1, 256);
        probe_dec_shape_kernel<2, 256, false, true><<<g4, 256, 0, c->stream>>>(static_cast<const uint32_t *>(d_src), dst, n16);
        break;
    }
    default:
        return fail(err, BITNUC_UNSUPPORTED);
    }
#undef PROBE
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// ---- host-pointer entry points (synchronous; size dispatch: runtime.h on_host) -------------------
int bitnuc_encode(bitnuc_ctx *c, const uint8_t *seq, size_t len, uint64_t *out, size_t *n_words, bitnuc_err *err) {
    clear_err(err);
    if (n_words) *n_words = 0;
    if (len == 0) return BITNUC_OK; // 0 words (the reference panics there: packing/avx.rs:138)
    if (!seq || !out) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, len)) { // host_word.h: same words, same first-invalid-byte rule, no launch
        const long long bad = bitnuc_host::encode_small(seq, len, out);
        if (bad >= 0) {
            if (err) { memset(err, 0, sizeof *err); err->status = BITNUC_INVALID_BASE; err->byte = seq[bad]; err->index = (uint64_t)bad; }
            if (n_words) *n_words = (size_t)bad / 32;
            return BITNUC_INVALID_BASE;
        }
        if (n_words) *n_words = words_for(len);
        return BITNUC_OK;
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    // on INVALID_BASE the pipelined driver has still run every chunk and handed every chunk's words back, the scratch loop stopped at
    // the failing chunk: out[*n_words ..] is unspecified (include/bitnuc_hip.h), the words before the failing 32-base group are the
    // reference's Vec contents
    const EncodeJob job{c, seq, out, len};
    bitnuc_err e{};
    const int st = c->host_pipeline && len >= kPipeMin ? pipe_run(c, job, &e) : scratch_run(c, job, &e);
    if (err) *err = e;
    if (n_words) *n_words = st == BITNUC_OK ? words_for(len) : st == BITNUC_INVALID_BASE ? (size_t)(e.index / 32) : 0;
    return st;
}

int bitnuc_decode(bitnuc_ctx *c, const uint64_t *ebuf, size_t n_words, size_t n_bases, uint8_t *out, bitnuc_err *err) {
    clear_err(err);
    if (n_words < words_for(n_bases)) return fail(err, BITNUC_INVALID_LENGTH, n_bases);
    if (n_bases == 0) return BITNUC_OK;
    if (!ebuf || !out) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, n_bases, true)) {
        bitnuc_host::decode_small(ebuf, n_bases, out);
        return BITNUC_OK;
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    // like every host-pointer call: an InvalidBase latched by earlier asynchronous launches stays for the next bitnuc_ctx_sync
    // (decode itself latches nothing, but the pipeline's abort path drains the ring and would drop it)
    if (int st = flush_pending(c, err)) return st;
    const DecodeJob job{c, ebuf, out, n_bases};
    return c->host_pipeline && n_bases >= kPipeMin ? pipe_run(c, job, err) : scratch_run(c, job, err);
}
// ---- single-word API: host code; batches of one on the device when forced ----------------
int bitnuc_as_2bit(bitnuc_ctx *c, const uint8_t *seq, size_t len, uint64_t *out, bitnuc_err *err) {
    clear_err(err);
    if (len > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, len); // packing/naive.rs:5-7: before any base is looked at
    if (!out || (len && !seq)) return fail(err, BITNUC_UNSUPPORTED);
    if (c && c->force_gpu) return bitnuc_as_2bit_batch(c, seq, len, len ? len : 1, 1, out, err);
    uint64_t w = 0;
    const int bad = bitnuc_host::pack_word(seq, len, &w);
    if (bad >= 0) {
        if (err) { memset(err, 0, sizeof *err); err->status = BITNUC_INVALID_BASE; err->byte = seq[bad]; err->index = (uint64_t)bad; }
        return BITNUC_INVALID_BASE;
    }
    *out = w;
    return BITNUC_OK;
}

int bitnuc_from_2bit(bitnuc_ctx *c, uint64_t packed, size_t n, uint8_t *out, bitnuc_err *err) {
    clear_err(err);
    if (n > 32) return fail(err, BITNUC_INVALID_LENGTH, n); // unpacking/naive.rs:8-10
    if (n == 0) return BITNUC_OK;
    if (!out) return fail(err, BITNUC_UNSUPPORTED);
    if (c && c->force_gpu) return bitnuc_decode(c, &packed, 1, n, out, err);
    bitnuc_host::unpack_word(packed, n, out);
    return BITNUC_OK;
}

int bitnuc_hdist_scalar(bitnuc_ctx *c, uint64_t u, uint64_t v, size_t len, uint32_t *out, bitnuc_err *err) {
    clear_err(err);
    if (len > 32) return fail(err, BITNUC_INVALID_LENGTH, len); // hamming/scalar.rs:13-15
    if (!out) return fail(err, BITNUC_UNSUPPORTED);
    if (c && c->force_gpu) return bitnuc_hdist(c, &u, 1, &v, 1, len, out, err);
    *out = bitnuc_host::hdist_word(u, v, len);
    return BITNUC_OK;
}

// Diagnostic (bench.py's small_call_latency block): mean ns per call of the HOST path over `iters` calls on the
// reference's bench input (cyclic "ACGT", benches/simd_comparison.rs:4-7), timed here so that no binding overhead is in it.
// op: 0 as_2bit, 1 from_2bit, 2 encode, 3 decode, 4 hdist_scalar.  Returns < 0 on a bad argument.
double bitnuc_selftime_small(int op, size_t n, size_t iters) {
    if (iters == 0 || n == 0 || op < 0 || op > 4 || ((op == 0 || op == 1 || op == 4) && n > 32)) return -1.0;
    // only sizes the host path takes with ctx == NULL (everything here is called without a context)
    if (n >= kDefaultHostCutoffDecode || (op == 2 && n >= kDefaultHostCutoff)) return -1.0;
    std::vector<uint8_t> seq(n), back(n);
    for (size_t i = 0; i < n; ++i) seq[i] = "ACGT"[i & 3];
    std::vector<uint64_t> words(words_for(n) + 1);
    size_t nw = 0;
    bitnuc_err e;
    if (bitnuc_encode(nullptr, seq.data(), n, words.data(), &nw, &e) != BITNUC_OK) return -1.0;
    volatile uint64_t sink = 0;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (size_t it = 0; it < iters; ++it) {
        uint64_t w = 0;
        uint32_t d = 0;
        seq[0] = "AC"[it & 1]; // the input changes between calls: the compiler cannot hoist the work
        switch (op) {
        case 0: (void)bitnuc_as_2bit(nullptr, seq.data(), n, &w, &e); sink += w; break;
        case 1: (void)bitnuc_from_2bit(nullptr, words[0] ^ it, n, back.data(), &e); sink += back[0]; break;
        case 2: (void)bitnuc_encode(nullptr, seq.data(), n, words.data(), &nw, &e); sink += words[0]; break;
        case 3: words[0] ^= it & 3; (void)bitnuc_decode(nullptr, words.data(), nw, n, back.data(), &e); sink += back[0]; break;
        case 4: (void)bitnuc_hdist_scalar(nullptr, words[0] ^ it, words[0], n, &d, &e); sink += d; break;
        default: return -1.0;
        }
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    (void)sink;
    return ((double)(t1.tv_sec - t0.tv_sec) * 1e9 + (double)(t1.tv_nsec - t0.tv_nsec)) / (double)iters;
}

} // extern "C"
