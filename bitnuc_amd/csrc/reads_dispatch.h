// reads_dispatch.h -- the host side of the per-read matchers (bitnuc_reads_*), written once: WHERE the reads are (four layouts), WHAT is computed
// (four matchers), one chunk loop, and the two skeletons every entry point is an instantiation of (reads_async, reads_host).  Part of kmer.hip, which
// includes it once, behind its own helpers (dev_queries, host_queries, multi_work, ascii_skip, packed_skip, bounded_grid, fail_invalid_base, ...).
// Kernels: scan_reads_device.h, scan_reads_batch_device.h, scan_anchored_device.h, scan_edist_device.h, scan_edist_best_device.h; below the host cutoff:
// reads_*_host.h.  At the end: the indel-tolerant family's second stage (bitnuc_reads_edist_start*: scan_edist_start_device.h, edist_start_host.h), which
// shares the layouts and has a skeleton of its own, and the 3' adapter per read (bitnuc_reads_edist_adapter*: scan_edist_adapter_device.h,
// reads_edist_adapter_host.h), which has five outputs and a rule and a skeleton of its own as well.
#pragma once

namespace {

inline bool words_ok(const void *p) { return p && !(reinterpret_cast<uintptr_t>(p) & 7); } // packed words and offsets tables: there and 8-byte aligned

// the outputs of a call, or of a chunk in scratch: the best triple and, where the runner-up is asked for, the second one
struct ReadsOut { uint32_t *query, *pos; uint8_t *dist, *dist2 = nullptr; uint32_t *query2 = nullptr, *pos2 = nullptr; }; // query2 == nullptr: the best triple only

// ---- where the reads are: the four layouts.  A layout names the data and, ragged, its tables: in device memory (the asynchronous forms' arguments, a staged
// chunk) or in host memory (the host forms' arguments).  It owns its size check (check 3), its pointer checks, the bound on a read's length the no-window
// rules are judged on (longest), the windows the cutoff is judged on, the cut of a batch into chunks of whole reads (chunk_end) and the staging of one:
// stage() copies the reads [r0, r0 + m) into scratch 0 (ragged: their rebased tables through `tab` into scratch 4) and returns the same layout over
// device memory; *base is the chunk's first byte, the slot base of an ASCII chunk (the packed kernels validate nothing and take no slot).
inline int check_fixed_size(size_t read_len, size_t count, bitnuc_err *err) {
    constexpr size_t kLimit = (size_t)1 << 58;
    if (read_len >= 0xFFFFFFFFull) return fail(err, BITNUC_UNSUPPORTED, read_len);
    const size_t period = 32 * words_for(read_len); // >= read_len, < 2^33
    if (period && count > (kLimit - 1) / period) return fail(err, BITNUC_UNSUPPORTED, read_len);
    return BITNUC_OK;
}

// count reads of read_len bytes, back to back, at any alignment
struct FixedAscii {
    static constexpr bool packed = false, ragged = false;
    const uint8_t *data; size_t read_len;
    size_t stride() const { return read_len; }
    int check_size(size_t count, bitnuc_err *err) const { return check_fixed_size(read_len, count, err); }
    bool tables_ok() const { return true; }
    bool data_ok() const { return data != nullptr; }
    uint64_t longest() const { return read_len; }
    size_t windows(size_t count, size_t k) const { return multi_work(read_len - k + 1, count); }
    size_t chunk_end(size_t r0, size_t count) const {
        const size_t per = read_len < kHostChunk ? kHostChunk / read_len : 1;
        return count - r0 < per ? count : r0 + per;
    }
    int stage(bitnuc_ctx *c, size_t r0, size_t m, std::vector<uint64_t> &, FixedAscii *dev, unsigned long long *base, bitnuc_err *err) const {
        if (int st = ensure_scratch(c, 0, m * read_len + 64, err)) return st;
        HIPCHK(hipMemcpyAsync(c->scratch[0], data + r0 * read_len, m * read_len, hipMemcpyHostToDevice, c->stream));
        *dev = FixedAscii{c->scratch[0], read_len};
        *base = (unsigned long long)r0 * read_len;
        return BITNUC_OK;
    }
};

// count reads of ceil(read_len / 32) 8-byte aligned words each
struct FixedPacked {
    static constexpr bool packed = true, ragged = false;
    const uint64_t *data; size_t read_len;
    size_t stride() const { return words_for(read_len); }
    int check_size(size_t count, bitnuc_err *err) const { return check_fixed_size(read_len, count, err); }
    bool tables_ok() const { return true; }
    bool data_ok() const { return words_ok(data); }
    uint64_t longest() const { return read_len; }
    size_t windows(size_t count, size_t k) const { return multi_work(read_len - k + 1, count); }
    size_t chunk_end(size_t r0, size_t count) const {
        const size_t per = stride() < kPackedChunkWords ? kPackedChunkWords / stride() : 1;
        return count - r0 < per ? count : r0 + per;
    }
    int stage(bitnuc_ctx *c, size_t r0, size_t m, std::vector<uint64_t> &, FixedPacked *dev, unsigned long long *base, bitnuc_err *err) const {
        const size_t wpr = stride();
        if (int st = ensure_scratch(c, 0, m * wpr * 8, err)) return st;
        HIPCHK(hipMemcpyAsync(c->scratch[0], data + r0 * wpr, m * wpr * 8, hipMemcpyHostToDevice, c->stream));
        *dev = FixedPacked{reinterpret_cast<const uint64_t *>(c->scratch[0]), read_len};
        *base = 0;
        return BITNUC_OK;
    }
};

// Both ragged layouts.  total: the run's length in the data's unit (bytes, words): what a launch walks and check 3 reports.  bases: what check 3 bounds and
// the no-window rule is judged on.  The host forms start with both 0: their tables' validation bounds the totals, then bases = offsets[count].

// read r is the bytes offsets[r] .. offsets[r + 1] of data, at any alignment
struct RaggedAscii {
    static constexpr bool packed = false, ragged = true;
    const uint8_t *data; const uint64_t *offsets; uint64_t total = 0, bases = 0;
    const uint64_t *starts() const { return nullptr; }
    int check_size(size_t, bitnuc_err *err) const { return bases >= ((uint64_t)1 << 58) ? fail(err, BITNUC_UNSUPPORTED, total) : BITNUC_OK; }
    bool tables_ok() const { return words_ok(offsets); }
    bool data_ok() const { return data != nullptr; }
    uint64_t longest() const { return bases; }
    size_t windows(size_t count, size_t k) const { return batch_windows(offsets, count, k); }
    BatchFault check_tables(size_t count) const { return batch_check_tables(offsets, nullptr, count); }
    size_t chunk_end(size_t r0, size_t count) const {
        return batch_chunk_end(r0, count, kHostChunk, [&](size_t a, size_t b) { return offsets[b] - offsets[a]; });
    }
    size_t chunk_size(size_t r0, size_t m) const { return (size_t)(offsets[r0 + m] - offsets[r0]); } // bytes
    long long chunk_first_invalid(size_t r0, size_t m) const {
        for (size_t i = (size_t)offsets[r0]; i < (size_t)offsets[r0 + m]; ++i) {
            const unsigned u = data[i] & 0xDFu;
            if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
        }
        return -1;
    }
    int stage(bitnuc_ctx *c, size_t r0, size_t m, std::vector<uint64_t> &tab, RaggedAscii *dev, unsigned long long *base, bitnuc_err *err) const {
        const size_t b0 = (size_t)offsets[r0], bytes = chunk_size(r0, m);
        if (int st = ensure_scratch(c, 0, bytes + 64, err)) return st;
        if (int st = ensure_scratch(c, 4, (m + 1) * 8, err)) return st;
        tab.resize(m + 1);
        for (size_t i = 0; i <= m; ++i) tab[i] = offsets[r0 + i] - b0;
        HIPCHK(hipMemcpyAsync(c->scratch[0], data + b0, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->scratch[4], tab.data(), (m + 1) * 8, hipMemcpyHostToDevice, c->stream));
        *dev = RaggedAscii{c->scratch[0], reinterpret_cast<const uint64_t *>(c->scratch[4]), bytes, bytes};
        *base = b0;
        return BITNUC_OK;
    }
};

// read r is the offsets[r + 1] - offsets[r] bases from word word_offsets[r] of data (encode_batch's tables), 8-byte aligned
struct RaggedPacked {
    static constexpr bool packed = true, ragged = true;
    const uint64_t *data, *word_offsets, *offsets; uint64_t total = 0, bases = 0;
    // in device memory (the asynchronous forms): check 3 bounds 32 x total_words, saturated from 2^53 words on, and reports total_words
    static RaggedPacked on_device(const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t total_words) {
        return RaggedPacked{d_words, d_word_offsets, d_offsets, total_words, total_words >= ((uint64_t)1 << 53) ? ~(uint64_t)0 : 32 * (uint64_t)total_words};
    }
    const uint64_t *starts() const { return word_offsets; }
    int check_size(size_t, bitnuc_err *err) const { return bases >= ((uint64_t)1 << 58) ? fail(err, BITNUC_UNSUPPORTED, total) : BITNUC_OK; }
    bool tables_ok() const { return words_ok(word_offsets) && words_ok(offsets); }
    bool data_ok() const { return words_ok(data); }
    uint64_t longest() const { return bases; }
    size_t windows(size_t count, size_t k) const { return batch_windows(offsets, count, k); }
    BatchFault check_tables(size_t count) const { return batch_check_tables(offsets, word_offsets, count); }
    size_t chunk_end(size_t r0, size_t count) const {
        return batch_chunk_end(r0, count, kPackedChunkWords, [&](size_t a, size_t b) { return word_offsets[b] - word_offsets[a]; });
    }
    size_t chunk_size(size_t r0, size_t m) const { return (size_t)(word_offsets[r0 + m] - word_offsets[r0]); } // words
    int stage(bitnuc_ctx *c, size_t r0, size_t m, std::vector<uint64_t> &tab, RaggedPacked *dev, unsigned long long *base, bitnuc_err *err) const {
        const size_t w0 = (size_t)word_offsets[r0], nw = chunk_size(r0, m);
        if (int st = ensure_scratch(c, 0, nw * 8, err)) return st;
        if (int st = ensure_scratch(c, 4, 2 * (m + 1) * 8, err)) return st;
        tab.resize(2 * (m + 1)); // word_offsets, then offsets
        for (size_t i = 0; i <= m; ++i) tab[i] = word_offsets[r0 + i] - w0, tab[m + 1 + i] = offsets[r0 + i] - offsets[r0];
        HIPCHK(hipMemcpyAsync(c->scratch[0], data + w0, nw * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->scratch[4], tab.data(), 2 * (m + 1) * 8, hipMemcpyHostToDevice, c->stream));
        const uint64_t *d_tab = reinterpret_cast<const uint64_t *>(c->scratch[4]);
        *dev = RaggedPacked{reinterpret_cast<const uint64_t *>(c->scratch[0]), d_tab, d_tab + m + 1, nw, 32 * (uint64_t)nw};
        *base = 0;
        return BITNUC_OK;
    }
};

// ---- the launches: one per kernel family, over a layout in device memory -----------------------------------------------------------------------------
// The best match per read (scan_reads_device.h; ragged: scan_reads_batch_device.h, which takes the run's length and the layout's two tables instead of a
// period).  Context scratch 10 holds the per-read keys (one u64 per read, all-ones = no admissible window yet) and behind them the tables (one BestTable
// per query, built in-stream from d_queries); a launch recorded into a hipGraph keeps it (ensure_scratch: warm up with the same or larger (count,
// n_queries) before capturing).  The keys are set to all-ones first in the same stream, the waves take their per-read minima into them and
// reads_finish_kernel writes query[] / pos[] / dist[].  The grid: the best match's (one workgroup per CU at most x the query blocks); a batch whose
// period is below a segment, or too small for a round, spreads its windows over more workgroups.  With the runner-up (o.query2) two key arrays live
// there: keys1 with one spare entry (count + 1: the exclusion form's loads), then keys2, both set to all-ones by one memset; the second pass reads keys1
// and fills keys2, reads_finish2_kernel writes the six outputs.
inline ReadsGeom reads_geom(size_t period, size_t read_len, size_t k) { return ReadsGeom{period, (unsigned)(read_len - k), 1.0f / (float)period}; }

template <bool PACKED, class HQ>
int reads_setup(bitnuc_ctx *c, size_t k, size_t count, unsigned long long n, unsigned long long rounds, const HQ *d_queries, size_t nq, unsigned long long **keys,
                const BestTable **tabs, dim3 *grid, bitnuc_err *err, unsigned long long **keys2 = nullptr) {
    const size_t nkeys = keys2 ? 2 * count + 1 : count;
    const size_t kbytes = (nkeys * 8 + 255) & ~(size_t)255;
    if (int st = ensure_scratch(c, 10, kbytes + nq * sizeof(BestTable), err)) return st;
    *keys = reinterpret_cast<unsigned long long *>(c->scratch[10]);
    if (keys2) *keys2 = *keys + count + 1;
    BestTable *t = reinterpret_cast<BestTable *>(c->scratch[10] + kbytes);
    HIPCHK(hipMemsetAsync(*keys, 0xFF, nkeys * sizeof(uint64_t), c->stream));
    best_tables_kernel<PACKED><<<(unsigned)nq, 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)k, t);
    HIPCHK(hipGetLastError());
    *tabs = t;
    unsigned gx = bounded_grid(c, rounds, (kMultiBlock / 64) * kMultiRounds, kMultiGrid);
    const unsigned long long single = (n - (rounds << 10)) / (4ull * kMultiBlock) + 1; // one-window-per-thread windows: four per thread
    const unsigned want = (unsigned)(single < (unsigned long long)c->num_cu ? single : (unsigned long long)c->num_cu);
    if (want > gx) gx = want;
    *grid = dim3(gx, (unsigned)((nq + kMultiQB - 1) / kMultiQB), 1);
    return BITNUC_OK;
}

inline int reads_finish(bitnuc_ctx *c, const unsigned long long *keys, const unsigned long long *keys2, size_t count, const ReadsOut &o, bitnuc_err *err) {
    HIPCHK(hipGetLastError());
    const size_t want = (count + 255) / 256, cap = (size_t)c->num_cu * 8;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    if (o.query2) reads_finish2_kernel<<<grid, 256, 0, c->stream>>>(keys, keys2, count, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
    else reads_finish_kernel<<<grid, 256, 0, c->stream>>>(keys, count, o.query, o.pos, o.dist);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// 1 <= k <= read_len, count >= 1, nq >= 1 (ascii_skip).  o.query2: the runner-up's outputs as well -- the exclusion pass over the same reads (none with
// one query: keys2 stays all-ones, the fill)
template <class HQ>
int launch_reads_best(bitnuc_ctx *c, const FixedAscii &in, size_t count, size_t k, const HQ *d_queries, size_t nq, const ReadsOut &o, unsigned long long *slot,
                      bitnuc_err *err) {
    const unsigned skip = ascii_skip(in.data);
    const unsigned long long n = (unsigned long long)count * in.read_len;
    const unsigned long long rounds = in.read_len >= kReadsMinPeriod ? scan_rounds(n, skip) : 0;
    unsigned long long *keys, *keys2 = nullptr;
    const BestTable *tabs;
    dim3 grid;
    if (int st = reads_setup<false>(c, k, count, n, rounds, d_queries, nq, &keys, &tabs, &grid, err, o.query2 ? &keys2 : nullptr)) return st;
    const ReadsGeom g = reads_geom(in.read_len, in.read_len, k);
    reads_best_kernel<kMultiRounds, false><<<grid, kMultiBlock, 0, c->stream>>>(in.data, n, skip, rounds, (unsigned)k, g, dev_queries(d_queries), (unsigned)nq, tabs, keys,
                                                                               slot);
    if (o.query2 && nq > 1) {
        HIPCHK(hipGetLastError());
        reads_best_kernel<kMultiRounds, true><<<grid, kMultiBlock, 0, c->stream>>>(in.data, n, skip, rounds, (unsigned)k, g, dev_queries(d_queries), (unsigned)nq, tabs,
                                                                                  keys, nullptr); // (keys2 == keys + count + 1: the kernel's own sum)
    }
    return reads_finish(c, keys, keys2, count, o, err);
}

// (packed_skip): the period is a whole number of words
template <class HQ>
int launch_reads_best(bitnuc_ctx *c, const FixedPacked &in, size_t count, size_t k, const HQ *d_queries, size_t nq, const ReadsOut &o, unsigned long long *,
                      bitnuc_err *err) {
    const unsigned skip = packed_skip(in.data);
    const size_t period = 32 * in.stride();
    const unsigned long long n = (unsigned long long)count * period;
    const unsigned long long rounds = scan_rounds(n, skip);
    unsigned long long *keys, *keys2 = nullptr;
    const BestTable *tabs;
    dim3 grid;
    if (int st = reads_setup<true>(c, k, count, n, rounds, d_queries, nq, &keys, &tabs, &grid, err, o.query2 ? &keys2 : nullptr)) return st;
    const ReadsGeom g = reads_geom(period, in.read_len, k);
    reads_best_packed_kernel<false><<<grid, kMultiBlock, 0, c->stream>>>(in.data, n, skip, rounds, (unsigned)k, g, dev_queries(d_queries), (unsigned)nq, tabs, keys);
    if (o.query2 && nq > 1) {
        HIPCHK(hipGetLastError());
        reads_best_packed_kernel<true><<<grid, kMultiBlock, 0, c->stream>>>(in.data, n, skip, rounds, (unsigned)k, g, dev_queries(d_queries), (unsigned)nq, tabs, keys);
    }
    return reads_finish(c, keys, keys2, count, o, err);
}

inline BatchTables batch_tables(const uint64_t *starts, const uint64_t *offsets, size_t count, unsigned shift) {
    return BatchTables{reinterpret_cast<const unsigned long long *>(starts), reinterpret_cast<const unsigned long long *>(offsets), count, shift};
}

// 1 <= k <= in.total, count >= 1, nq >= 1 (ascii_skip); the best triple only
template <class HQ>
int launch_reads_best(bitnuc_ctx *c, const RaggedAscii &in, size_t count, size_t k, const HQ *d_queries, size_t nq, const ReadsOut &o, unsigned long long *slot,
                      bitnuc_err *err) {
    const unsigned skip = ascii_skip(in.data);
    const unsigned long long n = in.total, rounds = scan_rounds(n, skip);
    unsigned long long *keys;
    const BestTable *tabs;
    dim3 grid;
    if (int st = reads_setup<false>(c, k, count, n, rounds, d_queries, nq, &keys, &tabs, &grid, err)) return st;
    reads_batch_kernel<kMultiRounds><<<grid, kMultiBlock, 0, c->stream>>>(in.data, batch_tables(in.offsets, in.offsets, count, 0), n, skip, rounds, (unsigned)k,
                                                                         dev_queries(d_queries), (unsigned)nq, tabs, keys, slot);
    return reads_finish(c, keys, nullptr, count, o, err);
}

// (packed_skip); in.total >= 1 words
template <class HQ>
int launch_reads_best(bitnuc_ctx *c, const RaggedPacked &in, size_t count, size_t k, const HQ *d_queries, size_t nq, const ReadsOut &o, unsigned long long *,
                      bitnuc_err *err) {
    const unsigned skip = packed_skip(in.data);
    const unsigned long long n = 32ull * in.total, rounds = scan_rounds(n, skip);
    unsigned long long *keys;
    const BestTable *tabs;
    dim3 grid;
    if (int st = reads_setup<true>(c, k, count, n, rounds, d_queries, nq, &keys, &tabs, &grid, err)) return st;
    reads_batch_packed_kernel<<<grid, kMultiBlock, 0, c->stream>>>(in.data, batch_tables(in.word_offsets, in.offsets, count, 5), n, skip, rounds, (unsigned)k,
                                                                   dev_queries(d_queries), (unsigned)nq, tabs, keys);
    return reads_finish(c, keys, nullptr, count, o, err);
}

// The ANCHORED best match and runner-up per read (scan_anchored_device.h): one kernel writes the six outputs, under the layout policy of its geometry --
// AnchorGeom, a stride per read, or AnchorBatchGeom, the ragged layouts' tables and the end the range is counted from.  lg: log2 of the rows per query.
template <class L>
auto anchor_geom(const L &in, int anchor, size_t pos_lo, size_t offsets, size_t k, size_t nq, unsigned lg, unsigned ntiles) {
    if constexpr (L::ragged)
        return AnchorBatchGeom{reinterpret_cast<const unsigned long long *>(in.offsets), reinterpret_cast<const unsigned long long *>(in.starts()), (unsigned)pos_lo,
                               (unsigned)(anchor == BITNUC_ANCHOR_END), (unsigned)(offsets + k - 1), (unsigned)offsets, lg, (unsigned)k, (unsigned)nq, ntiles};
    else
        return AnchorGeom{(unsigned long long)in.stride(), (unsigned)pos_lo, (unsigned)(offsets + k - 1), (unsigned)offsets, lg, (unsigned)k, (unsigned)nq, ntiles};
}

// Context scratch: the per-query tables only (256 bytes per query, after the best match's in scratch 10, shared with it in stream order).  count, nq,
// offsets >= 1, offsets + k - 1 <= 64; ragged: pos_lo < 2^32 - 1
template <class L, class HQ>
int launch_reads_anchored(bitnuc_ctx *c, const L &in, size_t count, size_t k, int anchor, size_t pos_lo, size_t offsets, const HQ *d_queries, size_t nq, const ReadsOut &o,
                          unsigned long long *slot, bitnuc_err *err) {
    if (int st = ensure_scratch(c, 10, nq * kAnchorEntry, err)) return st;
    anchored_tables_kernel<<<(unsigned)nq, 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)k, reinterpret_cast<uint32_t *>(c->scratch[10]));
    HIPCHK(hipGetLastError());
    unsigned lg = 0;
    while (((size_t)1 << lg) < offsets) ++lg;
    auto g = anchor_geom(in, anchor, pos_lo, offsets, k, nq, lg, (unsigned)(((nq << lg) + 31) >> 5));
    const size_t want = (count + 255) / 256, cap = (size_t)c->num_cu * 4; // 64 reads per wave and trip
    reads_anchored_kernel<L::packed, decltype(g)><<<(unsigned)(want < cap ? want : cap), kAnchorBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.data), (unsigned long long)count, g, c->scratch[10], o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// The INDEL-TOLERANT anchored best match and runner-up per read (scan_edist_device.h): a vector-ALU kernel, one read per lane, writes the six outputs;
// o.pos / o.pos2 hold the ends.  Context scratch: 16 bytes per query (scratch 10 again).  The ragged policy is the anchored kernel's geometry without
// rows; count, nq, k >= 1, k <= offsets + k - 1 <= 64
template <class L>
auto edist_geom(const L &in, int anchor, size_t pos_lo, size_t offsets, size_t k, size_t nq) {
    if constexpr (L::ragged) return anchor_geom(in, anchor, pos_lo, offsets, k, nq, 0u, 0u);
    else return EdistGeom{(unsigned long long)in.stride(), (unsigned)pos_lo, (unsigned)(offsets + k - 1), (unsigned)k, (unsigned)nq};
}

template <class L, class HQ>
int launch_reads_edist(bitnuc_ctx *c, const L &in, size_t count, size_t k, int anchor, size_t pos_lo, size_t offsets, const HQ *d_queries, size_t nq, const ReadsOut &o,
                       unsigned long long *slot, bitnuc_err *err) {
    if (int st = ensure_scratch(c, 10, nq * kEdistEntry, err)) return st;
    u32x4 *tabs = reinterpret_cast<u32x4 *>(c->scratch[10]);
    edist_tables_kernel<<<(unsigned)((nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)nq, (unsigned)k, tabs);
    HIPCHK(hipGetLastError());
    auto g = edist_geom(in, anchor, pos_lo, offsets, k, nq);
    const size_t want = (count + kEdistBlock - 1) / kEdistBlock, cap = (size_t)c->num_cu * kEdistBlocksPerCu;
    reads_edist_kernel<L::packed, decltype(g)><<<(unsigned)(want < cap ? want : cap), kEdistBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.data), (unsigned long long)count, g, tabs, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// The INDEL-TOLERANT best match and runner-up per read over the WHOLE read (scan_edist_best_device.h): the kernel above with the span's bound lifted, the
// lane walks its read in pieces of 64 bases.  Context scratch: 16 bytes per query (scratch 10 again).  The ragged policy is the anchored kernel's geometry
// with the whole read as the window (START, pos_lo = 0, every offset).  count, nq, k >= 1; reads of at most kEdistBestMaxRead bases; fixed: k <= read_len
template <class L>
auto edist_best_geom(const L &in, size_t k, size_t nq) {
    if constexpr (L::ragged)
        return AnchorBatchGeom{reinterpret_cast<const unsigned long long *>(in.offsets), reinterpret_cast<const unsigned long long *>(in.starts()), 0u, 0u, 0xFFFFFFFFu,
                               0xFFFFFFFFu, 0u, (unsigned)k, (unsigned)nq, 0u};
    else return EdistBestGeom{(unsigned long long)in.stride(), (unsigned)in.read_len, (unsigned)k, (unsigned)nq};
}

template <class L, class HQ>
int launch_reads_edist_best(bitnuc_ctx *c, const L &in, size_t count, size_t k, const HQ *d_queries, size_t nq, const ReadsOut &o, unsigned long long *slot,
                            bitnuc_err *err) {
    if (int st = ensure_scratch(c, 10, nq * kEdistEntry, err)) return st;
    u32x4 *tabs = reinterpret_cast<u32x4 *>(c->scratch[10]);
    edist_tables_kernel<<<(unsigned)((nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)nq, (unsigned)k, tabs);
    HIPCHK(hipGetLastError());
    auto g = edist_best_geom(in, k, nq);
    const size_t want = (count + kEdistBlock - 1) / kEdistBlock, cap = (size_t)c->num_cu * kEdistBlocksPerCu;
    reads_edist_best_kernel<L::packed, decltype(g)><<<(unsigned)(want < cap ? want : cap), kEdistBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.data), (unsigned long long)count, g, tabs, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// ---- what is computed: the matchers.  A matcher holds the call's k, queries and outputs and owns its part of the checks (needs_second, check_range), its
// no-window rule (no_window, on the layout's longest()), its bound on a validated table's lengths (check_lengths: the ragged host forms), the work its host cutoff is judged on, its host form below the cutoff (small: the index of the
// first invalid byte, or -1) and its launch over a layout in device memory.  whole_reads: every byte of every read is examined, also in a chunk that
// holds no window.

// the whole-read best match, with the runner-up where `second` (bitnuc_reads_*_best2*: its triple must be there)
template <class HQ> struct BestMatch {
    using Query = HQ;
    static constexpr bool whole_reads = true;
    size_t k; const HQ *queries; size_t nq; ReadsOut o; bool second;
    bool needs_second() const { return second; }
    template <class L> int check_range(const L &, bitnuc_err *) { return BITNUC_OK; }
    template <class L> int check_lengths(const L &, size_t, bitnuc_err *) const { return BITNUC_OK; }
    bool no_window(uint64_t longest) const { return k == 0 || nq == 0 || longest < k; }
    template <class L> size_t work(const L &in, size_t count) const { return multi_work(in.windows(count, k), nq); } // windows x queries, saturated
    long long small(const FixedAscii &in, size_t count) const {
        if (second)
            return reads_hdist_best2_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        return reads_hdist_best_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist);
    }
    long long small(const FixedPacked &in, size_t count) const {
        if (second) reads_hdist_best2_packed_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        else reads_hdist_best_packed_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist);
        return -1;
    }
    long long small(const RaggedAscii &in, size_t count) const {
        return reads_hdist_best_batch_small(in.data, in.offsets, count, k, host_queries(queries), nq, o.query, o.pos, o.dist);
    }
    long long small(const RaggedPacked &in, size_t count) const {
        reads_hdist_best_batch_packed_small(in.data, in.word_offsets, in.offsets, count, k, host_queries(queries), nq, o.query, o.pos, o.dist);
        return -1;
    }
    template <class L>
    int launch(bitnuc_ctx *c, const L &dev, size_t count, const HQ *d_queries, const ReadsOut &d, unsigned long long *slot, bitnuc_err *err) const {
        return launch_reads_best(c, dev, count, k, d_queries, nq, d, slot, err);
    }
};

// The anchored best match and runner-up: windows at the offsets pos_lo .. pos_hi only, counted in a ragged batch from the end `anchor` names.  EDIT: by
// edit distance instead of Hamming distance -- another launch, another host form, and the span (offsets + k - 1) where the Hamming form has the offsets.
template <class HQ, bool EDIT> struct AnchoredMatch {
    using Query = HQ;
    static constexpr bool whole_reads = false; // the spans only
    size_t k; const HQ *queries; size_t nq; ReadsOut o; int anchor; size_t pos_lo, pos_hi;
    size_t offsets = 0; // check_range's.  Ragged: pos_hi - pos_lo + 1, 0 for an empty range; fixed: those a read holds, 0 when none or without a query
    bool needs_second() const { return false; }
    template <class L> int check_range(const L &in, bitnuc_err *err) {
        size_t span = 0;
        if constexpr (L::ragged) {
            if (anchor != BITNUC_ANCHOR_START && anchor != BITNUC_ANCHOR_END) return fail(err, BITNUC_UNSUPPORTED, (uint64_t)(unsigned)anchor);
            anchored_batch_span(k, pos_lo, pos_hi, &offsets, &span);
        } else if (anchored_offsets(in.read_len, k, pos_lo, pos_hi, &offsets)) {
            span = offsets + k - 1;
        }
        if (span > BITNUC_ANCHOR_MAX_SPAN) return fail(err, BITNUC_UNSUPPORTED, span);
        if (!L::ragged && nq == 0) offsets = 0;
        return BITNUC_OK;
    }
    template <class L> int check_lengths(const L &, size_t, bitnuc_err *) const { return BITNUC_OK; }
    // no read of at most `longest` bases can hold a window: a window at offset pos_lo, or pos_lo bases in front of the end, needs k + pos_lo bases; reads
    // are below 2^32 - 1 bases.  (A fixed batch's offsets are 0 exactly when the other terms say so.)
    bool no_window(uint64_t longest) const {
        return k == 0 || nq == 0 || offsets == 0 || longest < k || longest - k < pos_lo || pos_lo >= 0xFFFFFFFFull;
    }
    size_t span() const { return EDIT ? offsets + k - 1 : offsets; }
    template <class L> size_t work(const L &, size_t count) const { return multi_work(multi_work(span(), count), nq); } // x queries, saturated
    long long small(const FixedAscii &in, size_t count) const {
        if constexpr (EDIT)
            return reads_edist_anchored_small(in.data, in.read_len, count, k, pos_lo, span(), host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        else
            return reads_hdist_anchored_small(in.data, in.read_len, count, k, pos_lo, span(), host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
    }
    long long small(const FixedPacked &in, size_t count) const {
        if constexpr (EDIT)
            reads_edist_anchored_packed_small(in.data, in.read_len, count, k, pos_lo, span(), host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        else
            reads_hdist_anchored_packed_small(in.data, in.read_len, count, k, pos_lo, span(), host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        return -1;
    }
    long long small(const RaggedAscii &in, size_t count) const {
        if constexpr (EDIT)
            return reads_edist_anchored_batch_small(in.data, in.offsets, count, k, anchor, pos_lo, pos_hi, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2,
                                                    o.dist2);
        else
            return reads_hdist_anchored_batch_small(in.data, in.offsets, count, k, anchor, pos_lo, pos_hi, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2,
                                                    o.dist2);
    }
    long long small(const RaggedPacked &in, size_t count) const {
        if constexpr (EDIT)
            reads_edist_anchored_batch_packed_small(in.data, in.word_offsets, in.offsets, count, k, anchor, pos_lo, pos_hi, host_queries(queries), nq, o.query, o.pos, o.dist,
                                                    o.query2, o.pos2, o.dist2);
        else
            reads_hdist_anchored_batch_packed_small(in.data, in.word_offsets, in.offsets, count, k, anchor, pos_lo, pos_hi, host_queries(queries), nq, o.query, o.pos, o.dist,
                                                    o.query2, o.pos2, o.dist2);
        return -1;
    }
    template <class L>
    int launch(bitnuc_ctx *c, const L &dev, size_t count, const HQ *d_queries, const ReadsOut &d, unsigned long long *slot, bitnuc_err *err) const {
        if constexpr (EDIT) return launch_reads_edist(c, dev, count, k, anchor, pos_lo, offsets, d_queries, nq, d, slot, err);
        else return launch_reads_anchored(c, dev, count, k, anchor, pos_lo, offsets, d_queries, nq, d, slot, err);
    }
};

// The indel-tolerant best match and runner-up over the WHOLE read: every read of at least k bases has a window, its whole length; a shorter read is neither
// read nor validated (whole_reads is false: a ragged ASCII chunk without a read of k bases is filled, not validated).  A read of more than
// BITNUC_EDIST_MAX_READ bases -> UNSUPPORTED (value = its length): fixed on read_len (check_range), ragged host forms at the table check (check_lengths)
template <class HQ> struct EditBestMatch {
    using Query = HQ;
    static constexpr bool whole_reads = false;
    size_t k; const HQ *queries; size_t nq; ReadsOut o;
    bool needs_second() const { return false; }
    template <class L> int check_range(const L &in, bitnuc_err *err) {
        if constexpr (!L::ragged)
            if (in.read_len > BITNUC_EDIST_MAX_READ) return fail(err, BITNUC_UNSUPPORTED, in.read_len);
        return BITNUC_OK;
    }
    template <class L> int check_lengths(const L &in, size_t count, bitnuc_err *err) const {
        for (size_t r = 0; r < count; ++r)
            if (in.offsets[r + 1] - in.offsets[r] > BITNUC_EDIST_MAX_READ) return fail(err, BITNUC_UNSUPPORTED, in.offsets[r + 1] - in.offsets[r]);
        return BITNUC_OK;
    }
    bool no_window(uint64_t longest) const { return k == 0 || nq == 0 || longest < k; }
    // (the bases of the reads with a window) x queries, saturated
    template <class L> size_t work(const L &in, size_t count) const {
        size_t bases = 0;
        if constexpr (L::ragged) {
            for (size_t r = 0; r < count; ++r) {
                const uint64_t len = in.offsets[r + 1] - in.offsets[r];
                if (len >= k) bases += (size_t)len; // below 2^58 in all
            }
        } else {
            bases = multi_work(in.read_len, count);
        }
        return multi_work(bases, nq);
    }
    long long small(const FixedAscii &in, size_t count) const {
        return reads_edist_best_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
    }
    long long small(const FixedPacked &in, size_t count) const {
        reads_edist_best_packed_small(in.data, in.read_len, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        return -1;
    }
    long long small(const RaggedAscii &in, size_t count) const {
        return reads_edist_best_batch_small(in.data, in.offsets, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
    }
    long long small(const RaggedPacked &in, size_t count) const {
        reads_edist_best_batch_packed_small(in.data, in.word_offsets, in.offsets, count, k, host_queries(queries), nq, o.query, o.pos, o.dist, o.query2, o.pos2, o.dist2);
        return -1;
    }
    template <class L>
    int launch(bitnuc_ctx *c, const L &dev, size_t count, const HQ *d_queries, const ReadsOut &d, unsigned long long *slot, bitnuc_err *err) const {
        return launch_reads_edist_best(c, dev, count, k, d_queries, nq, d, slot, err);
    }
};

// ---- the checks, the fills and the chunk loop every form shares -----------------------------------------------------------------------------------------
// The checks after ctx, in the header's order: k, the layout's sizes, the query limit, the matcher's range, count == 0 (*done: nothing to do, before any
// pointer is looked at), then the pointers: the best triple and the queries, the second triple (all three or none; all three where the matcher needs
// them), the layout's tables
template <class L, class M>
int check_reads(const L &in, size_t count, M &match, bool *done, bitnuc_err *err) {
    *done = false;
    if (match.k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, match.k);
    if (int st = in.check_size(count, err)) return st;
    if (match.nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, match.nq);
    if (int st = match.check_range(in, err)) return st;
    *done = count == 0;
    if (*done) return BITNUC_OK;
    const ReadsOut &o = match.o;
    const auto odd = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
    if (!o.query || !o.pos || !o.dist || odd(o.query) || odd(o.pos) || (!match.queries && match.nq) ||
        (reinterpret_cast<uintptr_t>(match.queries) & query_mask<typename M::Query>()))
        return fail(err, BITNUC_UNSUPPORTED);
    const int n2 = (o.query2 != nullptr) + (o.pos2 != nullptr) + (o.dist2 != nullptr);
    if ((n2 != 3 && (n2 != 0 || match.needs_second())) || odd(o.query2) || odd(o.pos2)) return fail(err, BITNUC_UNSUPPORTED);
    if (!in.tables_ok()) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// the ragged host forms' next check: batch_check_tables' finding as the call's error
inline int fail_batch_tables(const BatchFault &f, bitnuc_err *err) { return fail(err, f.kind >= 4 ? BITNUC_UNSUPPORTED : BITNUC_INVALID_RANGE, f.value); }

// no window: every read UINT32_MAX, UINT32_MAX, 0xFF, in both triples where there are two
inline void reads_fill_host(size_t count, const ReadsOut &o) {
    bitnuc_host::reads_best_fill(count, o.query, o.pos, o.dist);
    if (o.query2) bitnuc_host::reads_best_fill(count, o.query2, o.pos2, o.dist2);
}

inline int reads_fill_dev(bitnuc_ctx *c, size_t count, const ReadsOut &o, bitnuc_err *err) {
    HIPCHK(hipMemsetAsync(o.query, 0xFF, count * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(o.pos, 0xFF, count * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(o.dist, 0xFF, count, c->stream));
    return o.query2 ? reads_fill_dev(c, count, ReadsOut{o.query2, o.pos2, o.dist2}, err) : BITNUC_OK;
}

// The host forms' chunk loop: chunks of whole reads (no overlap: no window crosses a read), chunk_end(r0) is the read after the last of the chunk that
// starts at r0.  The queries are copied once into scratch 2; a chunk's query / pos arrays live in scratch 1, its distances in scratch 3 -- the second
// triple's behind the first's, neither computed nor copied where o has none -- and are copied straight to their place in the outputs: both triples are the
// chunk's own, nothing is merged across chunks.  launch(r0, m, d_queries, d) runs the reads [r0, r0 + m) into d's device arrays.  One drain per chunk;
// stops at the first failing chunk (its first invalid byte, absolute through the slot's base).
template <class HQ, class ChunkEnd, class Launch>
int reads_host_loop(bitnuc_ctx *c, size_t count, const HQ *queries, size_t nq, const ReadsOut &o, bitnuc_err *err, ChunkEnd chunk_end, Launch launch) {
    if (int st = ensure_scratch(c, 2, nq * sizeof(HQ), err)) return st; // 8: exact queries, 16: patterns
    HIPCHK(hipMemcpyAsync(c->scratch[2], queries, nq * sizeof(HQ), hipMemcpyHostToDevice, c->stream));
    const size_t triples = o.query2 ? 2 : 1;
    for (size_t r0 = 0; r0 < count;) {
        const size_t m = chunk_end(r0) - r0;
        if (int st = ensure_scratch(c, 1, triples * m * 8, err)) return st;
        if (int st = ensure_scratch(c, 3, triples * m < 64 ? 64 : triples * m, err)) return st;
        uint32_t *d_query = reinterpret_cast<uint32_t *>(c->scratch[1]), *d_pos = d_query + m;
        uint8_t *d_dist = c->scratch[3];
        const ReadsOut d = o.query2 ? ReadsOut{d_query, d_pos, d_dist, d_dist + m, d_pos + m, d_pos + 2 * m} : ReadsOut{d_query, d_pos, d_dist};
        if (int st = launch(r0, m, reinterpret_cast<const HQ *>(c->scratch[2]), d)) return st;
        HIPCHK(hipMemcpyAsync(o.query + r0, d.query, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o.pos + r0, d.pos, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o.dist + r0, d.dist, m, hipMemcpyDeviceToHost, c->stream));
        if (o.query2) {
            HIPCHK(hipMemcpyAsync(o.query2 + r0, d.query2, m * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(o.pos2 + r0, d.pos2, m * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(o.dist2 + r0, d.dist2, m, hipMemcpyDeviceToHost, c->stream));
        }
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        r0 += m;
    }
    return BITNUC_OK;
}

// ---- the two skeletons, over any layout and matcher ----------------------------------------------------------------------------------------------------
// an asynchronous form: everything in device memory, slot base 0
template <class L, class M>
int reads_async(bitnuc_ctx *c, const L &in, size_t count, M match, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    bool done;
    if (int st = check_reads(in, count, match, &done, err)) return st;
    if (done) return BITNUC_OK;
    DeviceGuard g(c->device);
    if (match.no_window(in.longest())) return reads_fill_dev(c, count, match.o, err);
    if (!in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    unsigned long long *slot = nullptr;
    if constexpr (!L::packed)
        if (int st = take_slot(c, 0, &slot, err)) return st;
    return match.launch(c, in, count, match.queries, match.o, slot, err);
}

// A host form: everything in host memory.  Ragged tables are validated before the fill and the data pointer check; below the cutoff the matcher's host
// form runs and no context is needed (check_ctx comes after it); above it the chunk loop stages and launches chunk by chunk.
template <class L, class M>
int reads_host(bitnuc_ctx *c, L in, size_t count, M match, bitnuc_err *err) {
    clear_err(err);
    bool done;
    if (int st = check_reads(in, count, match, &done, err)) return st;
    if (done) return BITNUC_OK;
    if constexpr (L::ragged) {
        const BatchFault f = in.check_tables(count);
        if (f.kind) return fail_batch_tables(f, err);
        if (int st = match.check_lengths(in, count, err)) return st;
        in.bases = in.offsets[count];
    }
    if (match.no_window(in.longest())) { reads_fill_host(count, match.o); return BITNUC_OK; }
    if (!in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, match.work(in, count))) {
        const long long bad = match.small(in, count);
        if constexpr (!L::packed)
            if (bad >= 0) return fail_invalid_base(err, in.data[bad], (uint64_t)bad);
        return BITNUC_OK;
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    std::vector<uint64_t> tab; // a ragged chunk's rebased tables on their way to scratch 4: alive until the chunk is drained
    return reads_host_loop(c, count, match.queries, match.nq, match.o, err, [&](size_t r0) { return in.chunk_end(r0, count); },
                           [&](size_t r0, size_t m, const typename M::Query *d_queries, const ReadsOut &d) {
        if constexpr (L::ragged) {
            // A chunk that holds no window launches nothing and is filled: an ASCII chunk by the matcher's rule on its bytes, a packed one without a
            // word.  A matcher of whole reads still validates the ASCII chunk's bytes, here.
            const size_t size = in.chunk_size(r0, m);
            if (L::packed ? size == 0 : match.no_window(size)) {
                if constexpr (!L::packed && M::whole_reads) {
                    const long long bad = in.chunk_first_invalid(r0, m);
                    if (bad >= 0) return fail_invalid_base(err, in.data[bad], (uint64_t)bad);
                }
                return reads_fill_dev(c, m, d, err);
            }
        }
        L dev{};
        unsigned long long base, *slot = nullptr;
        if (int st = in.stage(c, r0, m, tab, &dev, &base, err)) return st;
        if constexpr (!L::packed)
            if (int st = take_slot(c, base, &slot, err)) return st;
        return match.launch(c, dev, m, d_queries, d, slot, err);
    });
}

// ---- the forms behind the entry points, written once for both query kinds (HQ: uint64_t, bitnuc_reads_hdist_* / bitnuc_reads_edist_*; bitnuc_pattern,
// bitnuc_reads_pattern_*): each names its layout, its matcher and its skeleton.
template <class HQ>
int reads_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const HQ *d_queries, size_t n_queries,
                     uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_async(c, FixedAscii{d_reads, read_len}, count, BestMatch<HQ>{k, d_queries, n_queries, {d_best_query, d_best_pos, d_best_dist}, false}, err);
}
template <class HQ>
int reads_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const HQ *d_queries,
                            size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_async(c, FixedPacked{d_words, read_len}, count, BestMatch<HQ>{k, d_queries, n_queries, {d_best_query, d_best_pos, d_best_dist}, false}, err);
}
template <class HQ>
int reads_best_host(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries,
                    uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_host(c, FixedAscii{reads, read_len}, count, BestMatch<HQ>{k, queries, n_queries, {best_query, best_pos, best_dist}, false}, err);
}
template <class HQ>
int reads_best_packed_host(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries,
                           uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_host(c, FixedPacked{words, read_len}, count, BestMatch<HQ>{k, queries, n_queries, {best_query, best_pos, best_dist}, false}, err);
}

// ... and the runner-up
template <class HQ>
int reads_best2_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const HQ *d_queries, size_t n_queries,
                      uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos,
                      uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, FixedAscii{d_reads, read_len}, count, BestMatch<HQ>{k, d_queries, n_queries, o, true}, err);
}
template <class HQ>
int reads_best2_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const HQ *d_queries,
                             size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                             uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, FixedPacked{d_words, read_len}, count, BestMatch<HQ>{k, d_queries, n_queries, o, true}, err);
}
template <class HQ>
int reads_best2_host(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries,
                     uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                     bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, FixedAscii{reads, read_len}, count, BestMatch<HQ>{k, queries, n_queries, o, true}, err);
}
template <class HQ>
int reads_best2_packed_host(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries,
                            uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                            uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, FixedPacked{words, read_len}, count, BestMatch<HQ>{k, queries, n_queries, o, true}, err);
}

// the anchored forms of a fixed-length batch (the range counts from the reads' starts), by Hamming distance ...
template <class HQ>
int reads_anchored_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                         const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                         uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, FixedAscii{d_reads, read_len}, count, AnchoredMatch<HQ, false>{k, d_queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, FixedPacked{d_words, read_len}, count, AnchoredMatch<HQ, false>{k, d_queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_host(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const HQ *queries,
                        size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                        uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, FixedAscii{reads, read_len}, count, AnchoredMatch<HQ, false>{k, queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_packed_host(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                               const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                               uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, FixedPacked{words, read_len}, count, AnchoredMatch<HQ, false>{k, queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}

// ... and by edit distance: pos / pos2 are the ends
template <class HQ>
int reads_edist_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const HQ *d_queries,
                      size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                      uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, FixedAscii{d_reads, read_len}, count, AnchoredMatch<HQ, true>{k, d_queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const HQ *d_queries,
                             size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                             uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, FixedPacked{d_words, read_len}, count, AnchoredMatch<HQ, true>{k, d_queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_host(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const HQ *queries,
                     size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                     uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, FixedAscii{reads, read_len}, count, AnchoredMatch<HQ, true>{k, queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_packed_host(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const HQ *queries,
                            size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                            uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, FixedPacked{words, read_len}, count, AnchoredMatch<HQ, true>{k, queries, n_queries, o, BITNUC_ANCHOR_START, pos_lo, pos_hi}, err);
}

// the anchored forms of a ragged batch, by Hamming distance ...
template <class HQ>
int reads_anchored_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                               size_t pos_lo, size_t pos_hi, const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos,
                               uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, AnchoredMatch<HQ, false>{k, d_queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                      size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const HQ *d_queries, size_t n_queries,
                                      uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                      uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_pos, d_best_dist, d_second_dist, d_second_query, d_second_pos};
    return reads_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count,
                       AnchoredMatch<HQ, false>{k, d_queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_batch_host(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                              const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                              uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, RaggedAscii{seq, offsets}, count, AnchoredMatch<HQ, false>{k, queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_anchored_batch_packed_host(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                     int anchor, size_t pos_lo, size_t pos_hi, const HQ *queries, size_t n_queries, uint32_t *best_query,
                                     uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_pos, best_dist, second_dist, second_query, second_pos};
    return reads_host(c, RaggedPacked{words, word_offsets, offsets}, count, AnchoredMatch<HQ, false>{k, queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}

// ... and by edit distance
template <class HQ>
int reads_edist_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor, size_t pos_lo,
                            size_t pos_hi, const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                            uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, AnchoredMatch<HQ, true>{k, d_queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                   size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const HQ *d_queries, size_t n_queries,
                                   uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                   uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count,
                       AnchoredMatch<HQ, true>{k, d_queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_batch_host(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                           const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                           uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, RaggedAscii{seq, offsets}, count, AnchoredMatch<HQ, true>{k, queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}
template <class HQ>
int reads_edist_batch_packed_host(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int anchor,
                                  size_t pos_lo, size_t pos_hi, const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                  uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, RaggedPacked{words, word_offsets, offsets}, count, AnchoredMatch<HQ, true>{k, queries, n_queries, o, anchor, pos_lo, pos_hi}, err);
}

// the best match per read of a ragged batch
template <class HQ>
int reads_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                           const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count,
                       BestMatch<HQ>{k, d_queries, n_queries, {d_best_query, d_best_pos, d_best_dist}, false}, err);
}
template <class HQ>
int reads_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                  size_t total_words, size_t k, const HQ *d_queries, size_t n_queries, uint32_t *d_best_query,
                                  uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err) {
    return reads_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count,
                       BestMatch<HQ>{k, d_queries, n_queries, {d_best_query, d_best_pos, d_best_dist}, false}, err);
}
template <class HQ>
int reads_best_batch_host(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const HQ *queries, size_t n_queries,
                          uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_host(c, RaggedAscii{seq, offsets}, count, BestMatch<HQ>{k, queries, n_queries, {best_query, best_pos, best_dist}, false}, err);
}
template <class HQ>
int reads_best_batch_packed_host(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                 const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err) {
    return reads_host(c, RaggedPacked{words, word_offsets, offsets}, count, BestMatch<HQ>{k, queries, n_queries, {best_query, best_pos, best_dist}, false}, err);
}

// the indel-tolerant best match and runner-up over the whole read: fixed ...
template <class HQ>
int reads_edist_best_async(bitnuc_ctx *c, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const HQ *d_queries, size_t n_queries,
                           uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                           uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, FixedAscii{d_reads, read_len}, count, EditBestMatch<HQ>{k, d_queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_packed_async(bitnuc_ctx *c, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const HQ *d_queries, size_t n_queries,
                                  uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                  uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, FixedPacked{d_words, read_len}, count, EditBestMatch<HQ>{k, d_queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_host(bitnuc_ctx *c, const uint8_t *reads, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries, uint32_t *best_query,
                          uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, FixedAscii{reads, read_len}, count, EditBestMatch<HQ>{k, queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_packed_host(bitnuc_ctx *c, const uint64_t *words, size_t read_len, size_t count, size_t k, const HQ *queries, size_t n_queries,
                                 uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                 bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, FixedPacked{words, read_len}, count, EditBestMatch<HQ>{k, queries, n_queries, o}, err);
}

// ... and ragged
template <class HQ>
int reads_edist_best_batch_async(bitnuc_ctx *c, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, const HQ *d_queries,
                                 size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                 uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, RaggedAscii{d_seq, d_offsets, total_bases, total_bases}, count, EditBestMatch<HQ>{k, d_queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_batch_packed_async(bitnuc_ctx *c, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                        size_t total_words, size_t k, const HQ *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                        uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err) {
    const ReadsOut o{d_best_query, d_best_end, d_best_dist, d_second_dist, d_second_query, d_second_end};
    return reads_async(c, RaggedPacked::on_device(d_words, d_word_offsets, d_offsets, total_words), count, EditBestMatch<HQ>{k, d_queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_batch_host(bitnuc_ctx *c, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const HQ *queries, size_t n_queries,
                                uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, RaggedAscii{seq, offsets}, count, EditBestMatch<HQ>{k, queries, n_queries, o}, err);
}
template <class HQ>
int reads_edist_best_batch_packed_host(bitnuc_ctx *c, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                       const HQ *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                       uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err) {
    const ReadsOut o{best_query, best_end, best_dist, second_dist, second_query, second_end};
    return reads_host(c, RaggedPacked{words, word_offsets, offsets}, count, EditBestMatch<HQ>{k, queries, n_queries, o}, err);
}

// ---- the indel-tolerant family's second stage: WHERE the alignment that ends at end[r] starts (bitnuc_reads_edist_start*; scan_edist_start_device.h,
// below the host cutoff edist_start_host.h).  Not a fifth matcher of the skeletons above: it has two per-read INPUTS (query[], end[]) where a matcher has
// none, its outputs are (start, dist) and not a triple, and a read without bases still has an answer (e = 0: start 0, dist k), so a chunk without data is
// computed, not filled.  It shares the layouts -- their size check, pointer checks, chunks and staging -- and nothing of the four matchers changes.
template <class HQ> struct StartArgs {
    size_t k; int anchor; size_t pos; const HQ *queries; size_t nq; const uint32_t *query, *end; uint32_t *start; uint8_t *dist;
    bool reads_any() const { return k != 0 && nq != 0; } // otherwise every item is skipped: fills, nothing read, no data pointer looked at
    int from_end() const { return anchor == BITNUC_ANCHOR_END; }
};

// the checks after ctx, in the header's order: k, the layout's sizes, the query limit, the anchor, count == 0 (*done), then the pointers
template <class L, class HQ>
int check_reads_start(const L &in, size_t count, const StartArgs<HQ> &a, bool *done, bitnuc_err *err) {
    *done = false;
    if (a.k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, a.k);
    if (int st = in.check_size(count, err)) return st;
    if (a.nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, a.nq);
    if (a.anchor != BITNUC_ANCHOR_START && a.anchor != BITNUC_ANCHOR_END) return fail(err, BITNUC_UNSUPPORTED, (uint64_t)(unsigned)a.anchor);
    *done = count == 0;
    if (*done) return BITNUC_OK;
    const auto odd = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
    if (!a.query || !a.end || !a.start || odd(a.query) || odd(a.end) || odd(a.start) || (!a.queries && a.nq) ||
        (reinterpret_cast<uintptr_t>(a.queries) & query_mask<HQ>()))
        return fail(err, BITNUC_UNSUPPORTED);
    if (!in.tables_ok()) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

template <class L> auto start_geom(const L &in, int from_end, size_t pos, size_t k) {
    const unsigned p = pos < 0xFFFFFFFFull ? (unsigned)pos : 0xFFFFFFFFu; // reads are below 2^32 - 1 bases: no end reaches such a floor
    if constexpr (L::ragged)
        return StartBatchGeom{reinterpret_cast<const unsigned long long *>(in.offsets), reinterpret_cast<const unsigned long long *>(in.starts()), p, (unsigned)from_end,
                              (unsigned)k};
    else return StartFixedGeom{(unsigned long long)in.stride(), (unsigned)in.read_len, p, (unsigned)from_end, (unsigned)k};
}

// Context scratch: 16 bytes per query (scratch 10, the family's table slot, shared in stream order).  Everything in device memory; count >= 1 (start_grid:
// kmer.hip)
template <class L, class HQ>
int launch_reads_start(bitnuc_ctx *c, const L &in, size_t count, const StartArgs<HQ> &a, unsigned long long *slot, bitnuc_err *err) {
    u32x4 *tabs = nullptr;
    if (a.reads_any()) {
        if (int st = ensure_scratch(c, 10, a.nq * kEdistEntry, err)) return st;
        tabs = reinterpret_cast<u32x4 *>(c->scratch[10]);
        edist_tables_kernel<<<(unsigned)((a.nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(a.queries), (unsigned)a.nq, (unsigned)a.k, tabs);
        HIPCHK(hipGetLastError());
    }
    auto g = start_geom(in, a.from_end(), a.pos, a.k ? a.k : 1);
    edist_start_kernel<L::packed, decltype(g)><<<start_grid(c, count), kEdistBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.data), (unsigned long long)count, g, tabs, a.reads_any() ? (unsigned)a.nq : 0u, a.query, a.end, a.start, a.dist, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

template <class L, class HQ>
int reads_start_async(bitnuc_ctx *c, const L &in, size_t count, const StartArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    bool done;
    if (int st = check_reads_start(in, count, a, &done, err)) return st;
    if (done) return BITNUC_OK;
    if (a.reads_any() && !in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    DeviceGuard g(c->device);
    unsigned long long *slot = nullptr;
    if constexpr (!L::packed)
        if (a.reads_any())
            if (int st = take_slot(c, 0, &slot, err)) return st;
    return launch_reads_start(c, in, count, a, slot, err);
}

// the host form on the reads [r0, r0 + m): the index of the first invalid walked byte, or -1
template <class L, class HQ>
long long reads_start_small(const L &in, size_t r0, size_t m, const StartArgs<HQ> &a) {
    if constexpr (L::ragged) {
        const uint64_t *starts = in.starts();
        return reads_edist_start_batch_small<L::packed>(in.data, starts ? starts + r0 : nullptr, in.offsets + r0, m, a.k, a.from_end(), a.pos, host_queries(a.queries),
                                                        a.nq, a.query + r0, a.end + r0, a.start + r0, a.dist ? a.dist + r0 : nullptr);
    } else {
        const long long bad = reads_edist_start_small<L::packed>(in.data + r0 * in.stride(), in.read_len, m, a.k, a.from_end(), a.pos, host_queries(a.queries), a.nq,
                                                                 a.query + r0, a.end + r0, a.start + r0, a.dist ? a.dist + r0 : nullptr);
        return bad < 0 ? bad : bad + (long long)(r0 * in.stride());
    }
}

// Below the host cutoff (count x 2k, saturated) the host form runs and no context is needed; above it the layout's chunks of whole reads, with the
// chunk's query / end staged into scratch 1 and its start / dist staged out of scratch 1 / 3; the queries once in scratch 2
template <class L, class HQ>
int reads_start_host(bitnuc_ctx *c, L in, size_t count, const StartArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    bool done;
    if (int st = check_reads_start(in, count, a, &done, err)) return st;
    if (done) return BITNUC_OK;
    if constexpr (L::ragged) {
        const BatchFault f = in.check_tables(count);
        if (f.kind) return fail_batch_tables(f, err);
        in.bases = in.offsets[count];
    }
    if (a.reads_any() && !in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    if (!a.reads_any() || on_host(c, multi_work(count, 2 * a.k))) {
        const long long bad = reads_start_small(in, 0, count, a);
        if constexpr (!L::packed)
            if (bad >= 0) return fail_invalid_base(err, in.data[bad], (uint64_t)bad);
        return BITNUC_OK;
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    if (int st = ensure_scratch(c, 2, a.nq * sizeof(HQ), err)) return st;
    HIPCHK(hipMemcpyAsync(c->scratch[2], a.queries, a.nq * sizeof(HQ), hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> tab;
    for (size_t r0 = 0; r0 < count;) {
        const size_t m = in.chunk_end(r0, count) - r0;
        if constexpr (L::ragged) {
            if (in.chunk_size(r0, m) == 0) { // reads without a base: nothing to stage, e = 0 is their only end
                reads_start_small(in, r0, m, a);
                r0 += m;
                continue;
            }
        }
        if (int st = ensure_scratch(c, 1, 3 * m * 4, err)) return st;
        if (int st = ensure_scratch(c, 3, m < 64 ? 64 : m, err)) return st;
        uint32_t *d_query = reinterpret_cast<uint32_t *>(c->scratch[1]), *d_end = d_query + m, *d_start = d_end + m;
        HIPCHK(hipMemcpyAsync(d_query, a.query + r0, m * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_end, a.end + r0, m * 4, hipMemcpyHostToDevice, c->stream));
        L dev{};
        unsigned long long base, *slot = nullptr;
        if (int st = in.stage(c, r0, m, tab, &dev, &base, err)) return st;
        if constexpr (!L::packed)
            if (int st = take_slot(c, base, &slot, err)) return st;
        const StartArgs<HQ> d{a.k, a.anchor, a.pos, reinterpret_cast<const HQ *>(c->scratch[2]), a.nq, d_query, d_end, d_start, a.dist ? c->scratch[3] : nullptr};
        if (int st = launch_reads_start(c, dev, m, d, slot, err)) return st;
        HIPCHK(hipMemcpyAsync(a.start + r0, d_start, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (a.dist) HIPCHK(hipMemcpyAsync(a.dist + r0, c->scratch[3], m, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        r0 += m;
    }
    return BITNUC_OK;
}

// ---- the 3' ADAPTER per read (bitnuc_reads_edist_adapter*; scan_edist_adapter_device.h, below the host cutoff reads_edist_adapter_host.h): the whole-read
// matcher's layouts, limits, work and chunks with FIVE outputs and a rule (min_overlap, err_num / err_den).  A skeleton of its own, as the second stage
// has: ReadsOut is a pair of triples and stays one.
struct AdapterOut { uint32_t *adapter, *cut, *end; uint8_t *overlap, *dist; };

template <class HQ> struct AdapterArgs {
    size_t k; const HQ *queries; size_t nq, min_overlap, err_num, err_den; AdapterOut o;
    EditBestMatch<HQ> whole() const { return EditBestMatch<HQ>{k, queries, nq, ReadsOut{nullptr, nullptr, nullptr}}; } // its limits, no-window rule and work
};

// the checks after ctx, in the header's order: k, the layout's sizes, the query limit, the rule (k >= 1), the read length, count == 0 (*done), the pointers
template <class L, class HQ>
int check_reads_adapter(const L &in, size_t count, const AdapterArgs<HQ> &a, bool *done, bitnuc_err *err) {
    *done = false;
    if (a.k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, a.k);
    if (int st = in.check_size(count, err)) return st;
    if (a.nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, a.nq);
    if (a.k >= 1) {
        if (a.min_overlap == 0 || a.min_overlap > a.k) return fail(err, BITNUC_UNSUPPORTED, a.min_overlap);
        if (a.err_den == 0 || a.err_num > a.err_den) return fail(err, BITNUC_UNSUPPORTED, a.err_num);
    }
    if (int st = a.whole().check_range(in, err)) return st;
    *done = count == 0;
    if (*done) return BITNUC_OK;
    const auto odd = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
    const AdapterOut &o = a.o;
    if (!o.adapter || !o.cut || !o.end || !o.overlap || !o.dist || odd(o.adapter) || odd(o.cut) || odd(o.end) || (!a.queries && a.nq) ||
        (reinterpret_cast<uintptr_t>(a.queries) & query_mask<HQ>()))
        return fail(err, BITNUC_UNSUPPORTED);
    if (!in.tables_ok()) return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

inline void adapter_fill_host(size_t count, const AdapterOut &o) { bitnuc_host::adapter_fill(count, o.adapter, o.cut, o.end, o.overlap, o.dist); }

inline int adapter_fill_dev(bitnuc_ctx *c, size_t count, const AdapterOut &o, bitnuc_err *err) {
    HIPCHK(hipMemsetAsync(o.adapter, 0xFF, count * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(o.cut, 0xFF, count * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(o.end, 0xFF, count * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(o.overlap, 0xFF, count, c->stream));
    HIPCHK(hipMemsetAsync(o.dist, 0xFF, count, c->stream));
    return BITNUC_OK;
}

// Context scratch: 16 bytes per query (scratch 10, the family's table slot).  Everything in device memory; count, nq, k >= 1, 1 <= min_overlap <= k, reads of
// at most kEdistBestMaxRead bases; fixed: k <= read_len.  The rule travels by value in the geometry
template <class L, class HQ>
int launch_reads_adapter(bitnuc_ctx *c, const L &in, size_t count, const AdapterArgs<HQ> &a, const HQ *d_queries, const AdapterOut &o, unsigned long long *slot,
                         bitnuc_err *err) {
    if (int st = ensure_scratch(c, 10, a.nq * kEdistEntry, err)) return st;
    u32x4 *tabs = reinterpret_cast<u32x4 *>(c->scratch[10]);
    edist_tables_kernel<<<(unsigned)((a.nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(d_queries), (unsigned)a.nq, (unsigned)a.k, tabs);
    HIPCHK(hipGetLastError());
    const bitnuc_host::AdapterRule rule = bitnuc_host::adapter_rule(a.min_overlap, a.err_num, a.err_den);
    auto base = edist_best_geom(in, a.k, a.nq);
    uint32_t steps = 0; // bit i - 1: allowed(i) - allowed(i - 1), 0 or 1 since err_num <= err_den
    for (unsigned i = 1; i <= 32; ++i) steps |= (uint32_t)(rule.allowed[i] - rule.allowed[i - 1]) << (i - 1);
    const EdistAdapterGeom<decltype(base)> g{base, (unsigned)a.min_overlap, rule.allowed[a.k], steps};
    const size_t want = (count + kEdistBlock - 1) / kEdistBlock, cap = (size_t)c->num_cu * kEdistBlocksPerCu;
    reads_edist_adapter_kernel<L::packed, decltype(base)><<<(unsigned)(want < cap ? want : cap), kEdistBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.data), (unsigned long long)count, g, tabs, o.adapter, o.cut, o.end, o.overlap, o.dist, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

// an asynchronous form: everything in device memory, slot base 0
template <class L, class HQ>
int reads_adapter_async(bitnuc_ctx *c, const L &in, size_t count, const AdapterArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    bool done;
    if (int st = check_reads_adapter(in, count, a, &done, err)) return st;
    if (done) return BITNUC_OK;
    DeviceGuard g(c->device);
    if (a.whole().no_window(in.longest())) return adapter_fill_dev(c, count, a.o, err);
    if (!in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    unsigned long long *slot = nullptr;
    if constexpr (!L::packed)
        if (int st = take_slot(c, 0, &slot, err)) return st;
    return launch_reads_adapter(c, in, count, a, a.queries, a.o, slot, err);
}

// the host form on all reads: the index of the first invalid byte, or -1
template <class HQ> long long reads_adapter_small(const FixedAscii &in, size_t count, const AdapterArgs<HQ> &a, const bitnuc_host::AdapterRule &rule) {
    return reads_edist_adapter_small(in.data, in.read_len, count, a.k, host_queries(a.queries), a.nq, rule, a.o.adapter, a.o.cut, a.o.end, a.o.overlap, a.o.dist);
}
template <class HQ> long long reads_adapter_small(const FixedPacked &in, size_t count, const AdapterArgs<HQ> &a, const bitnuc_host::AdapterRule &rule) {
    reads_edist_adapter_packed_small(in.data, in.read_len, count, a.k, host_queries(a.queries), a.nq, rule, a.o.adapter, a.o.cut, a.o.end, a.o.overlap, a.o.dist);
    return -1;
}
template <class HQ> long long reads_adapter_small(const RaggedAscii &in, size_t count, const AdapterArgs<HQ> &a, const bitnuc_host::AdapterRule &rule) {
    return reads_edist_adapter_batch_small(in.data, in.offsets, count, a.k, host_queries(a.queries), a.nq, rule, a.o.adapter, a.o.cut, a.o.end, a.o.overlap, a.o.dist);
}
template <class HQ> long long reads_adapter_small(const RaggedPacked &in, size_t count, const AdapterArgs<HQ> &a, const bitnuc_host::AdapterRule &rule) {
    reads_edist_adapter_batch_packed_small(in.data, in.word_offsets, in.offsets, count, a.k, host_queries(a.queries), a.nq, rule, a.o.adapter, a.o.cut, a.o.end,
                                           a.o.overlap, a.o.dist);
    return -1;
}

// A host form: everything in host memory; reads_host's order (ragged tables validated, with the read length limit, before the fill and the data pointer
// check; below the cutoff the host form, ctx not needed; above it the layout's chunks of whole reads).  A chunk's adapter / cut / end live in scratch 1, its
// overlap / dist in scratch 3; the queries once in scratch 2.  A ragged chunk without a read of k bases launches nothing and is filled
template <class L, class HQ>
int reads_adapter_host(bitnuc_ctx *c, L in, size_t count, const AdapterArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    bool done;
    if (int st = check_reads_adapter(in, count, a, &done, err)) return st;
    if (done) return BITNUC_OK;
    const EditBestMatch<HQ> whole = a.whole();
    if constexpr (L::ragged) {
        const BatchFault f = in.check_tables(count);
        if (f.kind) return fail_batch_tables(f, err);
        if (int st = whole.check_lengths(in, count, err)) return st;
        in.bases = in.offsets[count];
    }
    if (whole.no_window(in.longest())) { adapter_fill_host(count, a.o); return BITNUC_OK; }
    if (!in.data_ok()) return fail(err, BITNUC_UNSUPPORTED);
    if (on_host(c, whole.work(in, count))) {
        const long long bad = reads_adapter_small(in, count, a, bitnuc_host::adapter_rule(a.min_overlap, a.err_num, a.err_den));
        if constexpr (!L::packed)
            if (bad >= 0) return fail_invalid_base(err, in.data[bad], (uint64_t)bad);
        return BITNUC_OK;
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard g(c->device);
    if (int st = flush_pending(c, err)) return st;
    if (int st = ensure_scratch(c, 2, a.nq * sizeof(HQ), err)) return st;
    HIPCHK(hipMemcpyAsync(c->scratch[2], a.queries, a.nq * sizeof(HQ), hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> tab; // a ragged chunk's rebased tables on their way to scratch 4: alive until the chunk is drained
    for (size_t r0 = 0; r0 < count;) {
        const size_t m = in.chunk_end(r0, count) - r0;
        const AdapterOut h{a.o.adapter + r0, a.o.cut + r0, a.o.end + r0, a.o.overlap + r0, a.o.dist + r0};
        if constexpr (L::ragged) {
            const size_t size = in.chunk_size(r0, m);
            if (L::packed ? size == 0 : whole.no_window(size)) {
                adapter_fill_host(m, h);
                r0 += m;
                continue;
            }
        }
        if (int st = ensure_scratch(c, 1, 3 * m * 4, err)) return st;
        if (int st = ensure_scratch(c, 3, 2 * m < 64 ? 64 : 2 * m, err)) return st;
        uint32_t *d_adapter = reinterpret_cast<uint32_t *>(c->scratch[1]);
        const AdapterOut d{d_adapter, d_adapter + m, d_adapter + 2 * m, c->scratch[3], c->scratch[3] + m};
        L dev{};
        unsigned long long base, *slot = nullptr;
        if (int st = in.stage(c, r0, m, tab, &dev, &base, err)) return st;
        if constexpr (!L::packed)
            if (int st = take_slot(c, base, &slot, err)) return st;
        if (int st = launch_reads_adapter(c, dev, m, a, reinterpret_cast<const HQ *>(c->scratch[2]), d, slot, err)) return st;
        HIPCHK(hipMemcpyAsync(h.adapter, d.adapter, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h.cut, d.cut, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h.end, d.end, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h.overlap, d.overlap, m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h.dist, d.dist, m, hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = drain(c, &e)) { if (err) *err = e; return st; }
        r0 += m;
    }
    return BITNUC_OK;
}

} // namespace
