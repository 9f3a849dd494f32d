// batch_launch.h -- the evidence build's dispatch of batch.hip's launchers: round 2's table-driven ragged batches (tile records by a
// search pre-kernel), the plan kernels at other block sizes, trip lengths, store policies and tilings with their timing-only
// ablations, the host-pointer ragged calls without a layout plan, and the fixed-length reads' other formulations.  Included once,
// by batch.hip inside an anonymous namespace, under -DBITNUC_SWEEP_VARIANTS.  Host code only; the kernels are in batch_evidence.h.
#pragma once

namespace evidence {

// ---- bitnuc_encode_batch_dev / bitnuc_decode_batch_dev: batch_tables_impl 0 ------------------------------------------------------
// rec[b] = {owner, first byte} of every 64-word wave tile, into context scratch (enqueued on the stream)
int batch_owners(bitnuc_ctx *c, const uint64_t *d_offsets, const uint64_t *d_word_offsets, size_t count, size_t total_words,
                 const TileRec **recs, bitnuc_err *err) {
    const size_t ntiles = (total_words + kBatchTile - 1) / kBatchTile;
    if (int st = ensure_scratch(c, 3, ntiles * sizeof(TileRec), err)) return st;
    TileRec *o = reinterpret_cast<TileRec *>(c->scratch[3]);
    const unsigned og = (unsigned)((ntiles + kBlock - 1) / kBlock);
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(d_offsets), *pw = reinterpret_cast<const unsigned long long *>(d_word_offsets);
    // count / total_words as a 0.64 fixed-point number (count <= total_words unless sequences are empty; saturate then)
    const unsigned long long ratio64 = count >= total_words ? ~0ull : (unsigned long long)((((unsigned __int128)count) << 64) / total_words);
    // measured (profiles/r01_ab_owner_estimate.txt): the multiply-high guess wins by 9 us of 17 for long sequences, the
    // 128-bit division by 6 of 28 for read-sized ones (same loads either way; the slower arithmetic spreads them out)
    const int est_mode = knobs(c).owner_est < 3 ? knobs(c).owner_est : (total_words >= 16 * (unsigned long long)count ? 2 : 0);
    if (est_mode == 0) block_owner_kernel<0><<<og, kBlock, 0, c->stream>>>(po, pw, count, total_words, ntiles, ratio64, o);
    else if (est_mode == 1) block_owner_kernel<1><<<og, kBlock, 0, c->stream>>>(po, pw, count, total_words, ntiles, ratio64, o);
    else block_owner_kernel<2><<<og, kBlock, 0, c->stream>>>(po, pw, count, total_words, ntiles, ratio64, o);
    HIPCHK(hipGetLastError());
    *recs = o;
    return BITNUC_OK;
}

bool wants_batch_tables(const bitnuc_ctx *c) { return knobs(c).batch_tables_impl != 1; }

// round 2's form: tile records by a search pre-kernel + O(1) window lookup inside the main kernel
int encode_batch_tables(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, const uint64_t *d_word_offsets, size_t count, size_t total_words,
                        uint64_t *d_out, bitnuc_err *err) {
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(d_offsets), *pw = reinterpret_cast<const unsigned long long *>(d_word_offsets);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(d_out);
    const TileRec *recs;
    if (int st = batch_owners(c, d_offsets, d_word_offsets, count, total_words, &recs, err)) return st;
    unsigned long long *slot;
    if (int st = take_slot(c, 0, &slot, err)) return st;
    const size_t per_block = (size_t)kBatchTile * kBatchWaves;
    const unsigned grid = grid_for(c, (total_words + per_block - 1) / per_block);
    switch (knobs(c).batch_abl) { // timing-only ablations (tools/ab_batch_ablate.py): anything but 0 produces wrong words
#define ABL_CASE(A) case A: encode_batch2_kernel<A><<<grid, kBlock, 0, c->stream>>>(d_seq, po, pw, count, total_words, recs, o, slot); break;
    ABL_CASE(1) ABL_CASE(2) ABL_CASE(3) ABL_CASE(8) ABL_CASE(9) ABL_CASE(11)
#undef ABL_CASE
    default: encode_batch2_kernel<0><<<grid, kBlock, 0, c->stream>>>(d_seq, po, pw, count, total_words, recs, o, slot);
    }
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

int decode_batch_tables(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words,
                        uint8_t *d_out, bitnuc_err *err) {
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(d_offsets), *pw = reinterpret_cast<const unsigned long long *>(d_word_offsets);
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(d_words);
    const TileRec *recs;
    if (int st = batch_owners(c, d_offsets, d_word_offsets, count, total_words, &recs, err)) return st;
    const size_t per_block = (size_t)kBatchTile * kBatchWaves;
    const unsigned grid = grid_for(c, (total_words + per_block - 1) / per_block);
    switch (knobs(c).batch_abl) {
#define ABL_CASE(A) case A: decode_batch2_kernel<A><<<grid, kBlock, 0, c->stream>>>(w, pw, po, count, total_words, recs, d_out); break;
    ABL_CASE(1) ABL_CASE(2) ABL_CASE(3) ABL_CASE(4) ABL_CASE(7) ABL_CASE(8) ABL_CASE(9) ABL_CASE(11) ABL_CASE(15)
#undef ABL_CASE
    default: decode_batch2_kernel<0><<<grid, kBlock, 0, c->stream>>>(w, pw, po, count, total_words, recs, d_out);
    }
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// ---- bitnuc_encode_batch / bitnuc_decode_batch: batch_host_plan 0 (the table-driven device calls instead of a layout plan) --------
bool wants_host_tables(const bitnuc_ctx *c) { return knobs(c).batch_host_plan == 0; }

// ---- launch_plan_encode ----------------------------------------------------------------------------------------------------------
bool wants_plan_encode(const bitnuc_ctx *c) {
    const SweepKnobs &s = knobs(c);
    return s.plan_enc_block != kPlanEncBlock || s.plan_enc_tiles != kPlanEncTiles || s.plan_enc_abl != 0;
}

int launch_plan_encode(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const unsigned long long *d_bounds,
                       const uint8_t *d_seq, unsigned long long *o, unsigned long long *slot, bitnuc_err *err) {
    const int threads = knobs(c).plan_enc_block, U = knobs(c).plan_enc_tiles;
#define PLAN_ENC(UU, A) plan_encode_t<UU, A>(c, d_base, d_P, total_words, d_bounds, d_seq, o, slot, threads)
    if (U == 2) HIPCHK(PLAN_ENC(2, 0));
    else if (U == 4) HIPCHK(PLAN_ENC(4, 0));
    else switch (knobs(c).plan_enc_abl) { // timing-only ablations, right only for 32-base reads (tools/ab_plan_enc_ablate.py)
    case 1: HIPCHK(PLAN_ENC(1, 1)); break;
    case 2: HIPCHK(PLAN_ENC(1, 2)); break;
    case 4: HIPCHK(PLAN_ENC(1, 4)); break;
    case 6: HIPCHK(PLAN_ENC(1, 6)); break;
    case 7: HIPCHK(PLAN_ENC(1, 7)); break;
    default: HIPCHK(PLAN_ENC(1, 0)); break;
    }
#undef PLAN_ENC
    return BITNUC_OK;
}

// ---- launch_plan_decode ----------------------------------------------------------------------------------------------------------
bool wants_plan_decode(const bitnuc_ctx *c) {
    const SweepKnobs &s = knobs(c);
    return s.plan_dec_lines != 0 || s.plan_tiles != kPlanTiles || s.plan_store != kPlanStore;
}

int launch_plan_decode(bitnuc_ctx *c, const unsigned long long *d_base, const uint8_t *d_P, size_t total_words, const unsigned long long *w,
                       uint8_t *d_out, bitnuc_err *err) {
    if (knobs(c).plan_dec_lines) { // line-owning tiles (batch_evidence.h; lost its A/B, profiles/r04_ab_plan_lines.txt): one tile per wave trip, the shipped store policy
        const unsigned grid = grid_for(c, (total_words + (size_t)kBatchTile * kBatchWaves - 1) / ((size_t)kBatchTile * kBatchWaves));
        if (knobs(c).plan_dec_lines == 2) decode_batch_plan_lines_kernel<2, 16><<<grid, kBlock, 0, c->stream>>>(w, d_base, d_P, total_words, d_out);
        else decode_batch_plan_lines_kernel<2, 128><<<grid, kBlock, 0, c->stream>>>(w, d_base, d_P, total_words, d_out);
        HIPCHK(hipGetLastError());
        return BITNUC_OK;
    }
    const int tiles = knobs(c).plan_tiles;
#define PLAN_DEC(POL) (tiles == 1 ? plan_decode_t<POL, 1>(c, d_base, d_P, total_words, w, d_out) : tiles == 2 ? plan_decode_t<POL, 2>(c, d_base, d_P, total_words, w, d_out) \
                                                                                                  : plan_decode_t<POL, 4>(c, d_base, d_P, total_words, w, d_out))
    HIPCHK(knobs(c).plan_store == 0 ? PLAN_DEC(0) : knobs(c).plan_store == 1 ? PLAN_DEC(1) : PLAN_DEC(2));
#undef PLAN_DEC
    return BITNUC_OK;
}

// ---- bitnuc_encode_fixed_dev / bitnuc_decode_fixed_dev: back-to-back reads (stride == read_len) ----------------------------------
bool wants_encode_fixed(const bitnuc_ctx *c, size_t read_len, size_t stride) { return stride == read_len && knobs(c).fixed_stream != kFixedStream; }

int launch_encode_fixed(bitnuc_ctx *c, unsigned grid, const uint8_t *d_seq, size_t read_len, unsigned wpr, unsigned magic, unsigned long long magic64,
                        unsigned long long total, unsigned long long seq_end, unsigned long long *o, unsigned long long *slot, bitnuc_err *err) {
    encode_fixed_kernel<false><<<grid, kBlock, 0, c->stream>>>(d_seq, (unsigned)read_len, read_len, wpr, magic, magic64, total, seq_end, knobs(c).fixed_stream, o, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// fixed_dec_strip: 0 = byte scatter, 1 = bit strip with per-lane 64-bit positions
bool wants_decode_fixed(const bitnuc_ctx *c, size_t read_len, size_t stride) { return stride == read_len && knobs(c).fixed_dec_strip != 2; }

int launch_decode_fixed(bitnuc_ctx *c, unsigned grid, const unsigned long long *w, size_t read_len, unsigned wpr, unsigned magic, unsigned long long magic64,
                        unsigned long long total, uint8_t *d_out, bitnuc_err *err) {
    if (knobs(c).fixed_dec_strip) decode_fixed_strip_kernel<<<grid, kBlock, 0, c->stream>>>(w, (unsigned)read_len, wpr, magic, magic64, total, d_out);
    else decode_fixed_kernel<true><<<grid, kBlock, 0, c->stream>>>(w, (unsigned)read_len, read_len, wpr, magic, magic64, total, d_out);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

} // namespace evidence
