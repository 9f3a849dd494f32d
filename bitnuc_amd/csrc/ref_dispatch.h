// ref_dispatch.h -- the host side of the searches along a reference (bitnuc_kmer_*: hit list, count, best match and histogram by Hamming distance; best
// match, count and hit list by edit distance), written once: WHERE the reference is (two inputs), WHAT is computed (one search per family, a template
// over the ABI's query type) and the two skeletons every one of the 56 entry points is an instantiation of (ref_async, ref_host).  Part of kmer.hip,
// which includes it once, behind the helpers it uses: the launchers and their argument structs, the check_* functions, the four chunk loops
// (multi_host_loop, best_host_loop, hist_host_loop, hits_host_loop), packed_chunk, multi_work, query_mask, no_windows, fail_invalid_base.
// Below the host cutoff: scan_hits_host.h, scan_multi_host.h, scan_best_host.h, scan_hist_host.h, kmer_edist_host.h.
#pragma once

namespace {

// ---- the geometry of a search: what a host chunk reports and the bases it needs around that.  Hamming: the windows [i, i + k), n - k + 1 of them; a
// chunk copies the k - 1 halo bases behind its last window.  Edit distance: the columns (ends), n of them; a chunk copies the 2k bases in front of its
// first column, which the launchers run but do not report (`lead`; packed: rounded up to whole words).
struct RefGeom { size_t units, halo, lead; };
template <bool EDIST> inline RefGeom ref_geom(size_t n, size_t k) { return EDIST ? RefGeom{n, 0, 2 * k} : RefGeom{n - k + 1, k - 1, 0}; }

// one host chunk staged in scratch 0: `bases` bases of which the first `lead` are overlap; slot: the chunk's error slot (nullptr: packed words hold no
// invalid base, so a packed chunk takes none)
struct RefChunk { const void *data; size_t bases, lead; unsigned long long *slot; };

// ---- where the reference is: the two inputs.  An input owns its length check (check 3), its data-pointer check, the units a host chunk reports (per),
// the size of scratch 0 and the staging of the chunk that reports the units [i0, i0 + per): the copy, then the slot at the base of the copy's first byte.
// n ASCII bytes at any alignment
struct AsciiRef {
    static constexpr bool packed = false;
    static constexpr size_t per = kHostChunk;
    const uint8_t *p; size_t n;
    int check_len(bitnuc_err *) const { return BITNUC_OK; }
    int check_ptr(bitnuc_err *err) const { return p ? BITNUC_OK : fail(err, BITNUC_UNSUPPORTED); }
    static size_t scratch_bytes(const RefGeom &) { return kHostChunk + 64; }
    int stage(bitnuc_ctx *c, const RefGeom &g, size_t i0, RefChunk *ch, bitnuc_err *err) const {
        const size_t m = g.units - i0 < per ? g.units - i0 : per, lead = i0 ? g.lead : 0; // i0 is 0 or at least kHostChunk
        HIPCHK(hipMemcpyAsync(c->scratch[0], p + i0 - lead, lead + m + g.halo, hipMemcpyHostToDevice, c->stream));
        unsigned long long *slot;
        if (int st = take_slot(c, i0 - lead, &slot, err)) return st;
        *ch = RefChunk{c->scratch[0], lead + m + g.halo, lead, slot};
        return BITNUC_OK;
    }
};

// n bases in n_words 8-byte aligned words; chunk i0 / 32 of whole words (packed_chunk) behind the words that hold its lead
struct PackedRef {
    static constexpr bool packed = true;
    static constexpr size_t per = 32 * kPackedChunkWords;
    const uint64_t *p; size_t n_words, n;
    int check_len(bitnuc_err *err) const { return n_words < words_for(n) ? fail(err, BITNUC_INVALID_LENGTH, n) : BITNUC_OK; }
    int check_ptr(bitnuc_err *err) const { return p && !(reinterpret_cast<uintptr_t>(p) & 7) ? BITNUC_OK : fail(err, BITNUC_UNSUPPORTED); }
    static size_t scratch_bytes(const RefGeom &g) { return (kPackedChunkWords + (g.lead ? 2 : 1)) * 8; }
    int stage(bitnuc_ctx *c, const RefGeom &g, size_t i0, RefChunk *ch, bitnuc_err *err) const {
        const PackedChunk pc = packed_chunk(i0 / 32, n, g.halo + 1);
        const size_t lw = i0 ? (g.lead + 31) / 32 : 0;
        HIPCHK(hipMemcpyAsync(c->scratch[0], p + pc.w0 - lw, (lw + pc.words) * 8, hipMemcpyHostToDevice, c->stream));
        *ch = RefChunk{c->scratch[0], 32 * lw + pc.bases, 32 * lw, nullptr};
        return BITNUC_OK;
    }
};

// ---- what is computed: one search per family, EDIST choosing the distance where a family has both.  A search holds the call's arguments and owns:
//   check(dev, none, err)   its argument checks (checks 4 ...; dev: an asynchronous form) and, where it has one, its "no queries -> OK" exit (*none)
//   fill_dev / fill_host    what a reference without windows leaves in the outputs
//   work(n, units)          what the host cutoff is judged on
//   small(ref / words)      its host form below the cutoff (ASCII: the index of the first invalid byte, or -1)
//   Args, args()            the launchers' argument struct over the call's own arrays
//   launch<PACKED>(...)     its launch on device data (`lead`: Hamming launches have none)
//   host_loop(..., f)       which chunk loop it runs; f(i0, a) stages and launches the chunk at i0 with the loop's device arrays
//   edist                   its geometry (ref_geom)
// the count of windows / ends within tau, per query
template <class HQ, bool EDIST> struct CountSearch {
    const HQ *queries; const uint32_t *taus; size_t nq; uint64_t *counts;
    using Args = MultiArgsT<HQ>;
    static constexpr bool edist = EDIST;
    int check(bool, bool *none, bitnuc_err *err) const { return check_multi(queries, taus, nq, counts, none, err, query_mask<HQ>()); }
    int fill_dev(bitnuc_ctx *c, bitnuc_err *err) const { HIPCHK(hipMemsetAsync(counts, 0, nq * sizeof(uint64_t), c->stream)); return BITNUC_OK; }
    void fill_host() const { memset(counts, 0, nq * sizeof(uint64_t)); }
    size_t work(size_t, size_t units) const { return multi_work(units, nq); }
    Args args() const { return Args{queries, taus, nq, reinterpret_cast<unsigned long long *>(counts)}; }
    template <bool PACKED>
    static int launch(bitnuc_ctx *c, const void *data, size_t n, size_t lead, size_t k, const Args &a, unsigned long long *slot, bitnuc_err *err) {
        if constexpr (EDIST) return launch_kmer_edist<PACKED, true>(c, data, n, lead, k, a.queries, a.taus, a.nq, a.counts, nullptr, slot, err);
        else if constexpr (PACKED) return launch_count_multi_packed(c, static_cast<const uint64_t *>(data), n, k, a, err);
        else return launch_count_multi(c, static_cast<const uint8_t *>(data), n, k, a, slot, err);
    }
    long long small(const uint8_t *ref, size_t n, size_t k) const {
        return EDIST ? bitnuc_host::kmer_edist_count_multi_small(ref, n, k, host_queries(queries), taus, nq, counts)
                     : bitnuc_host::kmer_hdist_count_multi_small(ref, n, k, host_queries(queries), taus, nq, counts);
    }
    void small(const uint64_t *words, size_t n, size_t k) const {
        if (EDIST) bitnuc_host::kmer_edist_count_multi_packed_small(words, n, k, host_queries(queries), taus, nq, counts);
        else bitnuc_host::kmer_hdist_count_multi_packed_small(words, n, k, host_queries(queries), taus, nq, counts);
    }
    template <class F> int host_loop(bitnuc_ctx *c, size_t units, size_t per, bitnuc_err *err, F f) const {
        return multi_host_loop(c, units, per, queries, taus, nq, counts, err, f);
    }
};

// the smallest distance and its leftmost window / end, per query
template <class HQ, bool EDIST> struct BestSearch {
    const HQ *queries; size_t nq; uint64_t *pos; uint8_t *dist;
    using Args = BestArgsT<HQ>;
    static constexpr bool edist = EDIST;
    int check(bool, bool *none, bitnuc_err *err) const { return check_best(queries, nq, pos, dist, none, err, query_mask<HQ>()); }
    int fill_dev(bitnuc_ctx *c, bitnuc_err *err) const { return best_fill_dev(c, pos, dist, nq, err); }
    void fill_host() const { memset(pos, 0xFF, nq * sizeof(uint64_t)); memset(dist, 0xFF, nq); }
    size_t work(size_t, size_t units) const { return multi_work(units, nq); }
    Args args() const { return Args{queries, nq, reinterpret_cast<unsigned long long *>(pos), dist}; }
    template <bool PACKED>
    static int launch(bitnuc_ctx *c, const void *data, size_t n, size_t lead, size_t k, const Args &a, unsigned long long *slot, bitnuc_err *err) {
        if constexpr (EDIST) return launch_kmer_edist<PACKED, false>(c, data, n, lead, k, a.queries, nullptr, a.nq, a.pos, a.dist, slot, err);
        else if constexpr (PACKED) return launch_best_packed(c, static_cast<const uint64_t *>(data), n, k, a, err);
        else return launch_best(c, static_cast<const uint8_t *>(data), n, k, a, slot, err);
    }
    long long small(const uint8_t *ref, size_t n, size_t k) const {
        return EDIST ? bitnuc_host::kmer_edist_best_small(ref, n, k, host_queries(queries), nq, pos, dist)
                     : bitnuc_host::kmer_hdist_best_small(ref, n, k, host_queries(queries), nq, pos, dist);
    }
    void small(const uint64_t *words, size_t n, size_t k) const {
        if (EDIST) bitnuc_host::kmer_edist_best_packed_small(words, n, k, host_queries(queries), nq, pos, dist);
        else bitnuc_host::kmer_hdist_best_packed_small(words, n, k, host_queries(queries), nq, pos, dist);
    }
    template <class F> int host_loop(bitnuc_ctx *c, size_t units, size_t per, bitnuc_err *err, F f) const {
        return best_host_loop(c, units, per, queries, nq, pos, dist, err, f);
    }
};

// the windows at each Hamming distance below n_bins, per query
template <class HQ> struct HistSearch {
    const HQ *queries; size_t nq, n_bins; uint64_t *hist;
    using Args = HistArgsT<HQ>;
    static constexpr bool edist = false;
    int check(bool, bool *none, bitnuc_err *err) const { return check_hist(queries, nq, n_bins, hist, none, err, query_mask<HQ>()); }
    int fill_dev(bitnuc_ctx *c, bitnuc_err *err) const { HIPCHK(hipMemsetAsync(hist, 0, nq * n_bins * sizeof(uint64_t), c->stream)); return BITNUC_OK; }
    void fill_host() const { memset(hist, 0, nq * n_bins * sizeof(uint64_t)); }
    size_t work(size_t, size_t units) const { return multi_work(units, nq); }
    Args args() const { return Args{queries, nq, n_bins, reinterpret_cast<unsigned long long *>(hist)}; }
    template <bool PACKED>
    static int launch(bitnuc_ctx *c, const void *data, size_t n, size_t, size_t k, const Args &a, unsigned long long *slot, bitnuc_err *err) {
        if constexpr (PACKED) return launch_hist_packed(c, static_cast<const uint64_t *>(data), n, k, a, err);
        else return launch_hist(c, static_cast<const uint8_t *>(data), n, k, a, slot, err);
    }
    long long small(const uint8_t *ref, size_t n, size_t k) const { return bitnuc_host::kmer_hdist_hist_small(ref, n, k, host_queries(queries), nq, n_bins, hist); }
    void small(const uint64_t *words, size_t n, size_t k) const { bitnuc_host::kmer_hdist_hist_packed_small(words, n, k, host_queries(queries), nq, n_bins, hist); }
    template <class F> int host_loop(bitnuc_ctx *c, size_t units, size_t per, bitnuc_err *err, F f) const {
        return hist_host_loop(c, units, per, queries, nq, n_bins, hist, err, f);
    }
};

// the positions (ends) within tau of ONE query, in ascending order, at most cap of them, and their number.  The query is a host value in every form: q
// points at the caller's pattern, or at the entry point's by-value argument.  The Hamming forms ask only that a pattern be there; the edit-distance
// forms ask of it what check_multi asks of a queries array of one.  The Hamming host forms take pos and n_hits at any alignment (host pointers);
// every other form goes through check_hits_out.  The cutoff is judged on the bases, one query.
template <class HQ, bool EDIST> struct HitsSearch {
    const HQ *q; unsigned tau; uint64_t *pos; uint8_t *hit_dist; size_t cap; uint64_t *n_hits;
    using Args = HitsArgsT<HQ>;
    static constexpr bool edist = EDIST;
    int check(bool dev, bool *, bitnuc_err *err) const {
        if (!q || (EDIST && (reinterpret_cast<uintptr_t>(q) & query_mask<HQ>()))) return fail(err, BITNUC_UNSUPPORTED);
        if (dev || EDIST) return check_hits_out(pos, cap, n_hits, err);
        return !n_hits || (!pos && cap) ? fail(err, BITNUC_UNSUPPORTED) : BITNUC_OK;
    }
    int fill_dev(bitnuc_ctx *c, bitnuc_err *err) const { HIPCHK(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), c->stream)); return BITNUC_OK; }
    void fill_host() const { *n_hits = 0; }
    size_t work(size_t n, size_t) const { return n; }
    Args args() const { return Args{*q, tau, reinterpret_cast<unsigned long long *>(pos), hit_dist, cap, reinterpret_cast<unsigned long long *>(n_hits), 0}; }
    template <bool PACKED>
    static int launch(bitnuc_ctx *c, const void *data, size_t n, size_t lead, size_t k, const Args &a, unsigned long long *slot, bitnuc_err *err) {
        if constexpr (EDIST) return launch_edist_hits<PACKED>(c, data, n, lead, k, a, slot, err);
        else if constexpr (PACKED) return launch_hits_packed(c, static_cast<const uint64_t *>(data), n, k, a, err);
        else return launch_hits(c, static_cast<const uint8_t *>(data), n, k, a, slot, err);
    }
    long long small(const uint8_t *ref, size_t n, size_t k) const {
        return EDIST ? bitnuc_host::kmer_edist_hits_small(ref, n, k, dev_query(*q), tau, pos, hit_dist, cap, n_hits)
                     : bitnuc_host::kmer_hdist_hits_small(ref, n, k, *host_queries(q), tau, pos, hit_dist, cap, n_hits);
    }
    void small(const uint64_t *words, size_t n, size_t k) const {
        *n_hits = EDIST ? bitnuc_host::kmer_edist_hits_packed_small(words, n, k, dev_query(*q), tau, pos, hit_dist, cap)
                        : bitnuc_host::kmer_hdist_hits_packed_small(words, n, k, *host_queries(q), tau, pos, hit_dist, cap);
    }
    template <class F> int host_loop(bitnuc_ctx *c, size_t units, size_t per, bitnuc_err *err, F f) const {
        return hits_host_loop(c, units, per, tau, *q, pos, hit_dist, cap, n_hits, err, [&](size_t i0, size_t, const Args &a) { return f(i0, a); });
    }
};

// the seven families
template <class HQ> using HdistHits = HitsSearch<HQ, false>;
template <class HQ> using HdistCount = CountSearch<HQ, false>;
template <class HQ> using HdistBest = BestSearch<HQ, false>;
template <class HQ> using HdistHist = HistSearch<HQ>;
template <class HQ> using EdistBest = BestSearch<HQ, true>;
template <class HQ> using EdistCount = CountSearch<HQ, true>;
template <class HQ> using EdistHits = HitsSearch<HQ, true>;

// ---- the two skeletons: the order every form shares.  Checks 1 - 3 (ctx, k, the packed word count), the search's own checks and its "no queries"
// exit, the fill when there is no window (nothing of the reference is looked at, not even its pointer), the data pointer, then the work.
// For k == 0 or n < k the edit-distance families keep the Hamming rule (no windows: the fill), although an end is defined for n < k.
template <class In, class S>
int ref_async(bitnuc_ctx *c, const In &in, size_t k, const S &s, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (int st = in.check_len(err)) return st;
    bool none = false;
    if (int st = s.check(true, &none, err)) return st;
    if (none) return BITNUC_OK;
    DeviceGuard g(c->device);
    if (no_windows(in.n, k)) return s.fill_dev(c, err);
    if (int st = in.check_ptr(err)) return st;
    unsigned long long *slot = nullptr;
    if constexpr (!In::packed) if (int st = take_slot(c, 0, &slot, err)) return st;
    return S::template launch<In::packed>(c, in.p, in.n, 0, k, s.args(), slot, err);
}

// The host forms need a context only above the cutoff: below it they are host code (a NULL context works).
template <class In, class S>
int ref_host(bitnuc_ctx *c, const In &in, size_t k, const S &s, bitnuc_err *err) {
    clear_err(err);
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (int st = in.check_len(err)) return st;
    bool none = false;
    if (int st = s.check(false, &none, err)) return st;
    if (none) return BITNUC_OK;
    if (no_windows(in.n, k)) { s.fill_host(); return BITNUC_OK; }
    if (int st = in.check_ptr(err)) return st;
    const RefGeom g = ref_geom<S::edist>(in.n, k);
    if (on_host(c, s.work(in.n, g.units))) {
        if constexpr (In::packed) { s.small(in.p, in.n, k); return BITNUC_OK; }
        else {
            const long long bad = s.small(in.p, in.n, k);
            return bad >= 0 ? fail_invalid_base(err, in.p[bad], (uint64_t)bad) : BITNUC_OK;
        }
    }
    if (int st = check_ctx(c, err)) return st;
    DeviceGuard guard(c->device);
    if (int st = flush_pending(c, err)) return st;
    if (int st = ensure_scratch(c, 0, In::scratch_bytes(g), err)) return st;
    return s.host_loop(c, g.units, In::per, err, [&](size_t i0, const typename S::Args &a) {
        RefChunk ch;
        if (int st = in.stage(c, g, i0, &ch, err)) return st;
        return S::template launch<In::packed>(c, ch.data, ch.bases, ch.lead, k, a, ch.slot, err);
    });
}

// ---- the indel-tolerant family's second stage along a reference: WHERE the alignments that end at end[0 .. m) start (bitnuc_ref_edist_start*;
// scan_edist_start_device.h, edist_start_host.h).  Not a search of the skeletons above: its work is m items of at most 63 bases each, not the reference,
// so there is no window rule, no chunking and no host cutoff -- the host forms always run on the host.  It shares the two inputs' checks.
template <class HQ> struct RefStartArgs {
    const HQ *queries; size_t nq; const uint32_t *query_index; const uint64_t *end; size_t m; const uint64_t *d_m; uint64_t *start; uint8_t *dist;
};

// the checks behind ctx, k and the word count: m == 0 (*done), the query limit, the pointers
template <class HQ>
int check_ref_start(const RefStartArgs<HQ> &a, bool *done, bitnuc_err *err) {
    *done = a.m == 0;
    if (*done) return BITNUC_OK;
    if (a.nq > BITNUC_MAX_QUERIES) return fail(err, BITNUC_UNSUPPORTED, a.nq);
    const auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (!a.end || !a.start || off(a.end, 7) || off(a.start, 7) || off(a.query_index, 3) || off(a.d_m, 7) || (!a.queries && a.nq) || off(a.queries, query_mask<HQ>()))
        return fail(err, BITNUC_UNSUPPORTED);
    return BITNUC_OK;
}

// Context scratch: 16 bytes per query in scratch 9, the slot the searches along a reference keep their tables in (shared in stream order)
template <class In, class HQ>
int ref_start_async(bitnuc_ctx *c, const In &in, size_t k, const RefStartArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    if (int st = check_ctx(c, err)) return st;
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (int st = in.check_len(err)) return st;
    bool done;
    if (int st = check_ref_start(a, &done, err)) return st;
    if (done) return BITNUC_OK;
    const bool reads_any = k != 0 && a.nq != 0; // otherwise every item is skipped: fills, nothing read
    if (reads_any)
        if (int st = in.check_ptr(err)) return st;
    DeviceGuard g(c->device);
    unsigned long long *slot = nullptr;
    u32x4 *tabs = nullptr;
    if (reads_any) {
        if constexpr (!In::packed) if (int st = take_slot(c, 0, &slot, err)) return st;
        if (int st = ensure_scratch(c, 9, a.nq * kEdistEntry, err)) return st;
        tabs = reinterpret_cast<u32x4 *>(c->scratch[9]);
        edist_tables_kernel<<<(unsigned)((a.nq + 63) / 64), 64, 0, c->stream>>>(dev_queries(a.queries), (unsigned)a.nq, (unsigned)k, tabs);
        HIPCHK(hipGetLastError());
    }
    const StartRefGeom geom{(unsigned long long)in.n, reinterpret_cast<const unsigned long long *>(a.d_m), (unsigned)(k ? k : 1)};
    edist_start_kernel<In::packed, StartRefGeom><<<start_grid(c, a.m), kEdistBlock, 0, c->stream>>>(
        reinterpret_cast<const uint8_t *>(in.p), (unsigned long long)a.m, geom, tabs, reads_any ? (unsigned)a.nq : 0u, a.query_index,
        reinterpret_cast<const unsigned long long *>(a.end), reinterpret_cast<unsigned long long *>(a.start), a.dist, slot);
    HIPCHK(hipGetLastError());
    return BITNUC_OK;
}

template <class In, class HQ>
int ref_start_host(const In &in, size_t k, const RefStartArgs<HQ> &a, bitnuc_err *err) {
    clear_err(err);
    if (k > 32) return fail(err, BITNUC_SEQUENCE_TOO_LONG, k);
    if (int st = in.check_len(err)) return st;
    bool done;
    if (int st = check_ref_start(a, &done, err)) return st;
    if (done) return BITNUC_OK;
    if (k != 0 && a.nq != 0)
        if (int st = in.check_ptr(err)) return st;
    const long long bad = bitnuc_host::kmer_edist_start_small<In::packed>(in.p, in.n, k, host_queries(a.queries), a.nq, a.query_index, a.end, a.m, a.start, a.dist);
    if constexpr (!In::packed)
        if (bad >= 0) return fail_invalid_base(err, in.p[bad], (uint64_t)bad);
    return BITNUC_OK;
}

} // namespace
