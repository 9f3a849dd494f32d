// batch.hip -- batches of independent sequences (reads, contigs) behind the C ABI (include/bitnuc_hip.h): ragged batches with
// offset tables, with a layout plan, and fixed-length reads.  The reference's user loops encode / decode over many short
// sequences, each call padding its own last word (src/utils/mod.rs:22-25,60-62, packing/avx.rs:147-148).  Kernels: batch_device.h.
#include "runtime.h"
#include "batch_device.h"
#include "host_pipe.h"

using namespace bitnuc_dev;
using namespace bitnuc_rt;

extern "C" {

static int check_offsets(const uint64_t *offsets, size_t count, bitnuc_err *err) {
    for (size_t i = 0; i < count; ++i)
        if (offsets[i + 1] < offsets[i]) { // argument check only (not codec arithmetic)
            if (err) { memset(err, 0, sizeof *err); err->status = BITNUC_INVALID_RANGE; err->value = i + 1; }
            return BITNUC_INVALID_RANGE;
        }
    return BITNUC_OK;
}

int bitnuc_batch_word_offsets_dev(bitnuc_ctx *c, const uint64_t *d_offsets, size_t count, uint64_t *d_word_offsets, size_t *total_words, bitnuc_err *err) {
    clear_err(err);
    if (total_words) *total_words = 0;
    if (int st = check_ctx(c, err)) return st;
    if (!d_word_offsets || (count && !d_offsets)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (count == 0) {
        HIPCHK(hipMemsetAsync(d_word_offsets, 0, sizeof(uint64_t), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return BITNUC_OK;
    }
    const size_t per_block = (size_t)kScanTile;
    const size_t nblocks = (count + per_block - 1) / per_block;
    if (int st = ensure_scratch(c, 3, (nblocks + 3) * sizeof(uint64_t), err)) return st;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(c->scratch[3]);
    const unsigned long long *off = reinterpret_cast<const unsigned long long *>(d_offsets);
    unsigned long long *wo = reinterpret_cast<unsigned long long *>(d_word_offsets);
    word_offsets_block_sums<<<(unsigned)nblocks, kBlock, 0, c->stream>>>(off, count, sums);
    word_offsets_scan_sums<<<1, kBlock, 0, c->stream>>>(sums, nblocks, off, count);
    word_offsets_finish<<<(unsigned)nblocks, kBlock, 0, c->stream>>>(off, count, sums, wo);
    HIPCHK(hipGetLastError());
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_word_offsets + count, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total_words) *total_words = (size_t)total;
    return BITNUC_OK;
}

// The table-driven forms.  Everything the layout plan depends on is in the caller's two tables and `total_words`, so ONE
// asynchronous launch (plan_emit_kernel: no scan, no host synchronisation, no memset) emits the plan's pad bytes, tile bases and
// buffer bounds into context scratch and the plan kernels do the work.  The scratch plan lives until the next table-driven call
// on this context (stream order).  Scratch grows on the first call / a larger batch (an allocation, which waits for the stream).
static int emit_scratch_plan(bitnuc_ctx *c, const uint64_t *d_offsets, const uint64_t *d_word_offsets, size_t count, size_t total_words,
                             uint8_t **P, unsigned long long **tile_base, unsigned long long **bounds, bitnuc_err *err) {
    const size_t ntiles = (total_words + kBatchTile - 1) / kBatchTile;
    if (int st = ensure_scratch(c, 6, total_words + 2 + kBatchTile, err)) return st;
    if (int st = ensure_scratch(c, 7, (ntiles + 1 + 2) * sizeof(unsigned long long), err)) return st;
    *P = c->scratch[6];
    *tile_base = reinterpret_cast<unsigned long long *>(c->scratch[7]);
    *bounds = *tile_base + ntiles + 1;
    const unsigned grid = (unsigned)((count + kScanTile - 1) / kScanTile);
    // word_offsets[i] is by definition the prefix sum of ceil(len / 32): the kernel reads one entry per workgroup and scans the rest
    plan_emit_kernel<true, false><<<grid, kBlock, 0, c->stream>>>(reinterpret_cast<const unsigned long long *>(d_offsets),
                                                                   reinterpret_cast<const unsigned long long *>(d_word_offsets), count, *P, *tile_base, *bounds, nullptr);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

} // extern "C"

// the plan kernels at a block size / trip length / store policy / ablation (the product: kPlanEncBlock, kPlanEncTiles, kPlanStore, kPlanTiles)
template <int U, int ABL>
static hipError_t plan_encode_t(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const unsigned long long *d_bounds,
                                const uint8_t *d_seq, unsigned long long *o, unsigned long long *slot, int threads) {
    const size_t per_block = (size_t)kBatchTile * (size_t)(threads / 64); // a wave owns a tile, so any number of waves per workgroup works
    const unsigned long long blocks = (total_words + per_block - 1) / per_block;
    encode_batch_plan_kernel<U, ABL><<<grid_for(c, (blocks + U - 1) / U, threads), threads, 0, c->stream>>>(d_seq, d_base, d_P, total_words, d_bounds, o, slot);
    return hipGetLastError();
}

template <int POL, int U>
static hipError_t plan_decode_t(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const unsigned long long *w, uint8_t *d_out) {
    const size_t per_block = (size_t)kBatchTile * kBatchWaves * U;
    decode_batch_plan_kernel<POL, U><<<grid_for(c, (total_words + per_block - 1) / per_block), kBlock, 0, c->stream>>>(w, d_base, d_P, total_words, d_out);
    return hipGetLastError();
}

#ifdef BITNUC_SWEEP_VARIANTS
namespace {
#include "evidence/batch_launch.h" // the formulations that lost their A/B: the hooks below
} // namespace
#endif

extern "C" {

static int launch_plan_encode(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const unsigned long long *d_bounds,
                              const uint8_t *d_seq, uint64_t *d_out, bitnuc_err *err) {
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    unsigned long long *o = reinterpret_cast<unsigned long long *>(d_out);
    BITNUC_EVIDENCE(if (evidence::wants_plan_encode(c)) return evidence::launch_plan_encode(c, d_base, d_P, total_words, d_bounds, d_seq, o, slot, err);)
    HIPCHK((plan_encode_t<kPlanEncTiles, 0>(c, d_base, d_P, total_words, d_bounds, d_seq, o, slot, kPlanEncBlock)));
    return BITNUC_OK;
}

static int launch_plan_decode(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const uint64_t *d_words,
                              uint8_t *d_out, bitnuc_err *err) {
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(d_words);
    BITNUC_EVIDENCE(if (evidence::wants_plan_decode(c)) return evidence::launch_plan_decode(c, d_base, d_P, total_words, w, d_out, err);)
    HIPCHK((plan_decode_t<kPlanStore, kPlanTiles>(c, d_base, d_P, total_words, w, d_out)));
    return BITNUC_OK;
}

int bitnuc_encode_batch_dev(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, const uint64_t *d_word_offsets, size_t count, size_t total_words, uint64_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || total_words == 0) return BITNUC_OK;
    if (!d_seq || !d_offsets || !d_word_offsets || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    BITNUC_EVIDENCE(if (evidence::wants_batch_tables(c)) return evidence::encode_batch_tables(c, d_seq, d_offsets, d_word_offsets, count, total_words, d_out, err);)
    uint8_t *P;
    unsigned long long *tile_base, *bounds;
    if (int st = emit_scratch_plan(c, d_offsets, d_word_offsets, count, total_words, &P, &tile_base, &bounds, err)) return st;
    return launch_plan_encode(c, tile_base, P, total_words, bounds, d_seq, d_out, err);
}

int bitnuc_decode_batch_dev(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, uint8_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || total_words == 0) return BITNUC_OK;
    if (!d_words || !d_offsets || !d_word_offsets || !d_out || (reinterpret_cast<uintptr_t>(d_words) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    BITNUC_EVIDENCE(if (evidence::wants_batch_tables(c)) return evidence::decode_batch_tables(c, d_words, d_word_offsets, d_offsets, count, total_words, d_out, err);)
    uint8_t *P;
    unsigned long long *tile_base, *bounds;
    if (int st = emit_scratch_plan(c, d_offsets, d_word_offsets, count, total_words, &P, &tile_base, &bounds, err)) return st;
    return launch_plan_decode(c, tile_base, P, total_words, d_words, d_out, err);
}

int bitnuc_encode_batch(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, uint64_t *out, size_t out_cap_words, uint64_t *word_offsets, size_t *n_words, bitnuc_err *err) {
    clear_err(err);
    if (n_words) *n_words = 0;
    if (int st = check_ctx(c, err)) return st;
    if (count == 0) { if (word_offsets) word_offsets[0] = 0; return BITNUC_OK; }
    if (!offsets || !word_offsets) return fail(err, BITNUC_UNSUPPORTED);
    if (int st = check_offsets(offsets, count, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    const uint64_t b0 = offsets[0], nbytes = offsets[count] - b0;
    if (int st = ensure_scratch(c, 0, nbytes + 16, err)) return st;
    if (int st = ensure_scratch(c, 4, (count + 1) * 8, err)) return st;
    uint64_t *d_off = reinterpret_cast<uint64_t *>(c->scratch[4]);
    if (nbytes && !seq) return fail(err, BITNUC_UNSUPPORTED);
    if (nbytes) HIPCHK(hipMemcpyAsync(c->scratch[0], seq + b0, nbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_off, offsets, (count + 1) * 8, hipMemcpyHostToDevice, c->stream));
    size_t total = 0;
    const uint64_t *d_wo;
    bool host_plan = true;
    BITNUC_EVIDENCE(host_plan = !evidence::wants_host_tables(c);)
    if (host_plan) { // the layout plan: word offsets + tile bases + pad bytes in one go (the context keeps one for its host calls)
        if (!c->host_plan) if (int st = bitnuc_batch_plan_create(c, &c->host_plan, err)) return st;
        if (int st = bitnuc_batch_plan_build_dev(c, c->host_plan, d_off, count, &total, err)) return st;
        d_wo = bitnuc_batch_plan_word_offsets_dev(c->host_plan);
    } else {
        if (int st = ensure_scratch(c, 5, (count + 1) * 8, err)) return st;
        if (int st = bitnuc_batch_word_offsets_dev(c, d_off, count, reinterpret_cast<uint64_t *>(c->scratch[5]), &total, err)) return st;
        d_wo = reinterpret_cast<const uint64_t *>(c->scratch[5]);
    }
    HIPCHK(hipMemcpyAsync(word_offsets, d_wo, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (total > out_cap_words || (total && !out)) { HIPCHK(hipStreamSynchronize(c->stream)); return fail(err, BITNUC_INVALID_LENGTH, total); }
    if (int st = ensure_scratch(c, 1, total * 8 + 16, err)) return st;
    // the kernels index the sequence buffer with the caller's offsets: rebase the device pointer
    const uint8_t *d_seq = c->scratch[0] - b0;
    if (total) {
        if (host_plan) { if (int st = bitnuc_encode_batch_plan_dev(c, c->host_plan, d_seq, reinterpret_cast<uint64_t *>(c->scratch[1]), err)) return st; }
        else if (int st = bitnuc_encode_batch_dev(c, d_seq, d_off, d_wo, count, total, reinterpret_cast<uint64_t *>(c->scratch[1]), err)) return st;
        HIPCHK(hipMemcpyAsync(out, c->scratch[1], total * 8, hipMemcpyDeviceToHost, c->stream));
    }
    bitnuc_err e;
    int st = drain(c, &e);
    if (st != BITNUC_OK) { if (err) *err = e; return st; }
    if (n_words) *n_words = total;
    return BITNUC_OK;
}

int bitnuc_decode_batch(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, uint8_t *out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0) return BITNUC_OK;
    if (!offsets || !word_offsets) return fail(err, BITNUC_UNSUPPORTED);
    if (int st = check_offsets(offsets, count, err)) return st;
    // the kernels index both buffers through these tables: a table that does not match the offsets
    // (word_offsets[i+1] - word_offsets[i] == ceil(len_i / 32), starting at 0) is refused here rather
    // than turned into an out-of-bounds device access (argument check only, not codec arithmetic)
    if (word_offsets[0] != 0) return fail(err, BITNUC_INVALID_RANGE, 0);
    for (size_t i = 0; i < count; ++i)
        if (word_offsets[i + 1] - word_offsets[i] != words_for((size_t)(offsets[i + 1] - offsets[i])) || word_offsets[i + 1] < word_offsets[i])
            return fail(err, BITNUC_INVALID_RANGE, i + 1);
    const uint64_t b0 = offsets[0], nbytes = offsets[count] - b0, total = word_offsets[count];
    if (total == 0) return BITNUC_OK;
    if (!words || !out) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (int st = ensure_scratch(c, 0, nbytes + 16, err)) return st;
    if (int st = ensure_scratch(c, 1, total * 8 + 16, err)) return st;
    if (int st = ensure_scratch(c, 4, (count + 1) * 8, err)) return st;
    if (int st = ensure_scratch(c, 5, (count + 1) * 8, err)) return st;
    uint64_t *d_off = reinterpret_cast<uint64_t *>(c->scratch[4]), *d_wo = reinterpret_cast<uint64_t *>(c->scratch[5]);
    HIPCHK(hipMemcpyAsync(c->scratch[1], words, total * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_off, offsets, (count + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_wo, word_offsets, (count + 1) * 8, hipMemcpyHostToDevice, c->stream));
    bool host_plan = true;
    BITNUC_EVIDENCE(host_plan = !evidence::wants_host_tables(c);)
    if (host_plan) { // the caller's word_offsets were checked against the offsets above; the plan rebuilds them on the device
        size_t ptotal = 0;
        if (!c->host_plan) if (int st = bitnuc_batch_plan_create(c, &c->host_plan, err)) return st;
        if (int st = bitnuc_batch_plan_build_dev(c, c->host_plan, d_off, count, &ptotal, err)) return st;
        if (ptotal != total) return fail(err, BITNUC_INVALID_RANGE, count);
        if (int st = bitnuc_decode_batch_plan_dev(c, c->host_plan, reinterpret_cast<const uint64_t *>(c->scratch[1]), c->scratch[0] - b0, err)) return st;
    } else if (int st = bitnuc_decode_batch_dev(c, reinterpret_cast<const uint64_t *>(c->scratch[1]), d_wo, d_off, count, total, c->scratch[0] - b0, err)) return st;
    HIPCHK(hipMemcpyAsync(out + b0, c->scratch[0], nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BITNUC_OK;
}

// ---- ragged batches with a layout plan --------------------------------------------------------------
struct bitnuc_batch_plan {
    int device = 0;
    size_t count = 0, total_words = 0;
    unsigned long long seq_begin = 0, seq_end = 0;
    unsigned long long *d_wo = nullptr;   // count + 1 word offsets
    unsigned long long *d_base = nullptr; // one byte offset per 64-word tile
    uint8_t *d_P = nullptr;               // total_words + 1 pad bytes
    unsigned long long *d_bounds = nullptr; // offsets[0], offsets[count] (what the plan encode clips its loads to)
    size_t cap_wo = 0, cap_base = 0, cap_P = 0, cap_bounds = 0;
    bool built = false;
};

int bitnuc_batch_plan_create(bitnuc_ctx *c, bitnuc_batch_plan **out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (!out) return fail(err, BITNUC_UNSUPPORTED);
    bitnuc_batch_plan *p = new bitnuc_batch_plan();
    p->device = c->device;
    *out = p;
    return BITNUC_OK;
}

void bitnuc_batch_plan_destroy(bitnuc_batch_plan *p) {
    if (!p) return;
    DeviceGuard g(p->device);
    if (p->d_wo) (void)hipFree(p->d_wo);
    if (p->d_base) (void)hipFree(p->d_base);
    if (p->d_P) (void)hipFree(p->d_P);
    if (p->d_bounds) (void)hipFree(p->d_bounds);
    delete p;
}

size_t bitnuc_batch_plan_total_words(const bitnuc_batch_plan *p) { return p && p->built ? p->total_words : 0; }
size_t bitnuc_batch_plan_count(const bitnuc_batch_plan *p) { return p && p->built ? p->count : 0; }
const uint64_t *bitnuc_batch_plan_word_offsets_dev(const bitnuc_batch_plan *p) { return p && p->built ? reinterpret_cast<const uint64_t *>(p->d_wo) : nullptr; }

extern "C++" {
namespace {
template <class T> int plan_reserve(T **buf, size_t *cap, size_t need_elems, hipStream_t stream, bitnuc_err *err) {
    if (need_elems <= *cap) return BITNUC_OK;
    if (*buf) {
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipFree(*buf));
        *buf = nullptr;
        *cap = 0;
    }
    size_t want = need_elems + need_elems / 4 + 64; // head-room: a stream of batches of similar size reuses the plan's memory
    if (hipMalloc(reinterpret_cast<void **>(buf), want * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        want = need_elems;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(buf), want * sizeof(T)));
    }
    *cap = want;
    return BITNUC_OK;
}
} // namespace
} // extern "C++"

int bitnuc_batch_plan_build_dev(bitnuc_ctx *c, bitnuc_batch_plan *p, const uint64_t *d_offsets, size_t count, size_t *total_words, bitnuc_err *err) {
    clear_err(err);
    if (total_words) *total_words = 0;
    if (int st = check_ctx(c, err)) return st;
    if (!p || p->device != c->device || (count && !d_offsets)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    p->built = false;
    if (int st = plan_reserve(&p->d_wo, &p->cap_wo, count + 1, c->stream, err)) return st;
    // sums -> scan of the sums -> (host learns the total and sizes the plan) -> offsets + pad bytes + tile bases + bounds in one pass
    unsigned long long ends[3] = {0, 0, 0}; // total words, offsets[0], offsets[count]
    const size_t nblocks = (count + kScanTile - 1) / kScanTile;
    const unsigned long long *off = reinterpret_cast<const unsigned long long *>(d_offsets);
    unsigned long long *sums = nullptr;
    if (count) {
        if (int st = ensure_scratch(c, 3, (nblocks + 3) * sizeof(uint64_t), err)) return st;
        sums = reinterpret_cast<unsigned long long *>(c->scratch[3]);
        word_offsets_block_sums<<<(unsigned)nblocks, kBlock, 0, c->stream>>>(off, count, sums);
        word_offsets_scan_sums<<<1, kBlock, 0, c->stream>>>(sums, nblocks, off, count);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ends, sums + nblocks, sizeof ends, hipMemcpyDeviceToHost, c->stream)); // total, offsets[0], offsets[count]
        HIPCHK(hipStreamSynchronize(c->stream));
    } else {
        HIPCHK(hipMemsetAsync(p->d_wo, 0, sizeof(uint64_t), c->stream));
    }
    const size_t total = (size_t)ends[0];
    p->count = count;
    p->total_words = total;
    const size_t ntiles = (total + kBatchTile - 1) / kBatchTile;
    if (int st = plan_reserve(&p->d_base, &p->cap_base, ntiles + 1, c->stream, err)) return st;
    if (int st = plan_reserve(&p->d_P, &p->cap_P, total + 2 + kBatchTile, c->stream, err)) return st;
    if (int st = plan_reserve(&p->d_bounds, &p->cap_bounds, 2, c->stream, err)) return st;
    if (count) { // one pass: word offsets + pad bytes + tile bases + buffer bounds (every pad byte is written: no memset)
        plan_emit_kernel<false, true><<<(unsigned)nblocks, kBlock, 0, c->stream>>>(off, sums, count, p->d_P, p->d_base, p->d_bounds, p->d_wo);
        HIPCHK(hipGetLastError());
    }
    p->seq_begin = ends[1];
    p->seq_end = ends[2];
    HIPCHK(hipStreamSynchronize(c->stream)); // the build is synchronous: the plan's tables may be read on any stream afterwards
    p->built = true;
    if (total_words) *total_words = total;
    return BITNUC_OK;
}

int bitnuc_encode_batch_plan_dev(bitnuc_ctx *c, const bitnuc_batch_plan *p, const uint8_t *d_seq, uint64_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (!p || !p->built || p->device != c->device) return fail(err, BITNUC_UNSUPPORTED);
    if (p->total_words == 0) return BITNUC_OK;
    if (!d_seq || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    return launch_plan_encode(c, p->d_base, p->d_P, p->total_words, p->d_bounds, d_seq, d_out, err);
}

int bitnuc_decode_batch_plan_dev(bitnuc_ctx *c, const bitnuc_batch_plan *p, const uint64_t *d_words, uint8_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (!p || !p->built || p->device != c->device) return fail(err, BITNUC_UNSUPPORTED);
    if (p->total_words == 0) return BITNUC_OK;
    if (!d_words || !d_out || (reinterpret_cast<uintptr_t>(d_words) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    return launch_plan_decode(c, p->d_base, p->d_P, p->total_words, d_words, d_out, err);
}

// ---- fixed-length reads ------------------------------------------------------------------------
int bitnuc_encode_fixed_dev(bitnuc_ctx *c, const uint8_t *d_seq, size_t read_len, size_t stride, size_t count, uint64_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || read_len == 0) return BITNUC_OK; // zero-length reads produce no words
    if (stride < read_len || read_len > 0xFFFFFFFFull - 64) return fail(err, BITNUC_UNSUPPORTED);
    if (!d_seq || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    const unsigned wpr = (unsigned)words_for(read_len);
    const unsigned long long total = (unsigned long long)count * wpr;
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    const size_t per_block = (size_t)kBatchTile * kBatchWaves;
    const unsigned grid = grid_for(c, (total + per_block - 1) / per_block);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(d_out);
    const unsigned long long seq_end = (unsigned long long)(count - 1) * stride + read_len;
    const unsigned magic = (unsigned)((0x100000000ull + wpr - 1) / wpr); // ceil(2^32 / wpr): exact floor(t / wpr) for t < 2^16
    const unsigned long long magic64 = wpr == 1 ? 0ull : ~0ull / wpr + 1;  // floor(2^64 / wpr) + 1: exact floor(w / wpr) by multiply-high while w * wpr < 2^64
    BITNUC_EVIDENCE(if (evidence::wants_encode_fixed(c, read_len, stride)) return evidence::launch_encode_fixed(c, grid, d_seq, read_len, wpr, magic, magic64, total, seq_end, o, slot, err);)
    if (stride == read_len) encode_fixed_kernel<false><<<grid, kBlock, 0, c->stream>>>(d_seq, (unsigned)read_len, stride, wpr, magic, magic64, total, seq_end, kFixedStream, o, slot);
    else encode_fixed_kernel<true><<<grid, kBlock, 0, c->stream>>>(d_seq, (unsigned)read_len, stride, wpr, magic, magic64, total, seq_end, 0, o, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

int bitnuc_decode_fixed_dev(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t stride, size_t count, uint8_t *d_out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || read_len == 0) return BITNUC_OK;
    if (stride < read_len || read_len > 0xFFFFFFFFull - 64) return fail(err, BITNUC_UNSUPPORTED);
    if (!d_words || !d_out || (reinterpret_cast<uintptr_t>(d_words) & 7)) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    const unsigned wpr = (unsigned)words_for(read_len);
    const unsigned long long total = (unsigned long long)count * wpr;
    const size_t per_block = (size_t)kBatchTile * kBatchWaves;
    const unsigned grid = grid_for(c, (total + per_block - 1) / per_block);
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(d_words);
    const unsigned magic = (unsigned)((0x100000000ull + wpr - 1) / wpr);
    const unsigned long long magic64 = wpr == 1 ? 0ull : ~0ull / wpr + 1;
    BITNUC_EVIDENCE(if (evidence::wants_decode_fixed(c, read_len, stride)) return evidence::launch_decode_fixed(c, grid, w, read_len, wpr, magic, magic64, total, d_out, err);)
    if (stride != read_len) decode_fixed_kernel<false><<<grid, kBlock, 0, c->stream>>>(w, (unsigned)read_len, stride, wpr, magic, magic64, total, d_out);
    else decode_fixed_tile_kernel<2><<<grid, kBlock, 0, c->stream>>>(w, (unsigned)read_len, wpr, magic, magic64, total, d_out); // back-to-back reads: the plan decode's tile body
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// Host-pointer fixed-length reads: a job of host_pipe.h whose items are reads.  A pipe chunk is as many whole reads as fit both
// buffers (their bytes in an A buffer, their words in a B buffer; decode the other way round).
namespace {
struct FixedJob {
    bitnuc_ctx *c; bool encode; const uint8_t *seq; const uint64_t *words; size_t read_len, stride, count; uint64_t *out_words; uint8_t *out_seq;
    int in_kind, out_kind;
    bool drains, inout; // encode latches errors; decode with separators copies the caller's bytes between reads in so they go back unchanged
    size_t wpr;
    FixedJob(bitnuc_ctx *c, bool encode, const uint8_t *seq, const uint64_t *words, size_t read_len, size_t stride, size_t count, uint64_t *out_words, uint8_t *out_seq)
        : c(c), encode(encode), seq(seq), words(words), read_len(read_len), stride(stride), count(count), out_words(out_words), out_seq(out_seq),
          in_kind(encode ? kBufA : kBufB), out_kind(encode ? kBufB : kBufA), drains(encode), inout(!encode && stride != read_len), wpr(words_for(read_len)) {}
    size_t pipe_per(size_t chunk) const { // 0 for a read larger than a chunk (today unreachable: the callers admit read_len, stride < 1 Mi)
        const size_t per = (chunk / 4) / (8 * wpr), by_bytes = chunk > read_len ? (chunk - read_len) / stride + 1 : 0;
        return by_bytes < per ? by_bytes : per;
    }
    size_t scratch_per() const { return kHostChunk / stride; }
    size_t seq_bytes(size_t m) const { return (m - 1) * stride + read_len; }
    const void *in_src(size_t i0) const { return encode ? static_cast<const void *>(seq + i0 * stride) : static_cast<const void *>(words + i0 * wpr); }
    size_t in_bytes(size_t m) const { return encode ? seq_bytes(m) : m * wpr * 8; }
    void *out_dst(size_t i0) const { return encode ? static_cast<void *>(out_words + i0 * wpr) : static_cast<void *>(out_seq + i0 * stride); }
    size_t out_bytes(size_t m) const { return encode ? m * wpr * 8 : seq_bytes(m); }
    int launch(size_t i0, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err) const {
        if (!encode) return bitnuc_decode_fixed_dev(c, reinterpret_cast<const uint64_t *>(d_in), read_len, stride, m, d_out, err);
        if (int st = bitnuc_encode_fixed_dev(c, d_in, read_len, stride, m, reinterpret_cast<uint64_t *>(d_out), err)) return st;
        set_last_slot_base(c, (unsigned long long)i0 * stride); // report the index in the caller's buffer
        return BITNUC_OK;
    }
};
} // namespace

int bitnuc_encode_fixed(bitnuc_ctx *c, const uint8_t *seq, size_t read_len, size_t stride, size_t count, uint64_t *out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || read_len == 0) return BITNUC_OK;
    if (stride < read_len || !seq || !out) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    const FixedJob job(c, true, seq, nullptr, read_len, stride, count, out, nullptr);
    return c->host_pipeline && (count - 1) * stride + read_len >= kPipeMin && stride < ((size_t)1 << 20) ? pipe_run(c, job, err) : scratch_run(c, job, err);
}

int bitnuc_decode_fixed(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t stride, size_t count, uint8_t *out, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (count == 0 || read_len == 0) return BITNUC_OK;
    if (stride < read_len || !words || !out) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    const FixedJob job(c, false, nullptr, words, read_len, stride, count, nullptr, out);
    // back-to-back reads only: with separators the bytes between reads are the caller's and would have to travel both ways
    if (c->host_pipeline && stride == read_len && count * read_len >= kPipeMin && read_len < ((size_t)1 << 20)) {
        if (int st = flush_pending(c, err)) return st;
        return pipe_run(c, job, err);
    }
    return scratch_run(c, job, err);
}

} // extern "C"
