"""GPU tests of the indel-tolerant family's second stage -- where the alignment that ends at a given base starts (bitnuc_reads_edist_start*_async,
bitnuc_ref_edist_start*_async, the pattern twins and the per-read host forms above the cutoff; edist_start_kernel, scan_edist_start_device.h) against
tests/edist_start_oracle.py (one Levenshtein table per candidate substring) and against the host forms.  One item per lane: the lane loads its own query's
table entry, gathers the w <= 63 bases in front of its end and walks them backwards; the loop is wave-uniform over the wave's largest w.  So: 333 reads
(more than a block, a partial last wave) of k .. 200 bases, ragged and fixed; windows that start at every byte of a dword and span 16 or 17 dwords; packed
windows in one, two and three words with ends at 0, 1 and 31 mod 32; a wave of equal w, waves of mixed w with w = 0 among them, a wave of skipped items;
every forward _async form followed by the start form; a hit list that feeds the start call through its device count; a queue without a sync between the
forward and the start calls; a hipGraph of forward + start replayed on new reads; invalid bytes; the host forms in one chunk and across two; references of
more than 2^32 bases.  Every comparison is exact equality; guard words and bytes surround the outputs, dist starts at an odd byte offset."""
import numpy as np
import pytest

import edist_start_oracle as so
import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
MARK32 = 0x5A5A5A5A
MARK64 = 0x5A5A5A5A5A5A5A5A
COUNT = 333


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def _dev_queries(queries, pattern):
    return _dev(rp.as_patterns(queries)) if pattern else _dev(np.asarray(queries, dtype=np.uint64).reshape(-1))


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


class Out:
    """start with GUARD words before and after [0, n) (u32 per read, u64 along a reference); dist inside a guarded buffer, starting at byte 3"""

    def __init__(self, n, wide=False):
        import torch
        self.n, self.wide = n, wide
        self.s = torch.full((n + 2 * GUARD,), MARK64 if wide else MARK32, dtype=torch.int64 if wide else torch.int32, device="cuda:0")
        self.d = torch.full((3 + n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")

    def ptrs(self):
        return self.s.data_ptr() + (8 if self.wide else 4) * GUARD, self.d.data_ptr() + 3

    def read(self, ctx, written=None):
        """the outputs after a sync; written: the items a device count allowed (default all) -- nothing else may be touched"""
        ctx.sync()
        n = self.n if written is None else written
        s = self.s.cpu().numpy().view(np.uint64 if self.wide else np.uint32)
        d = self.d.cpu().numpy()
        mark = MARK64 if self.wide else MARK32
        assert (s[:GUARD] == mark).all() and (s[GUARD + n:] == mark).all(), "start written outside its items"
        assert (d[:3] == 0x5A).all() and (d[3 + n:] == 0x5A).all(), "dist written outside its items"
        return s[GUARD:GUARD + n].copy(), d[3:3 + n].copy()


def _reads_data(layout, packed, s, shape, k, aoff=0):
    """the layout arguments of a per-read _async call in device memory -> (keep-alive, head); ASCII at byte offset aoff of its buffer, zeros around it"""
    import torch
    if layout == "fixed":
        count = s.size // shape if shape else 0
        if packed:
            w = _dev(ro.pack_reads(s, shape, count))
            return w, (w, shape, count)
        t = torch.zeros(s.size + aoff + 16, dtype=torch.uint8, device="cuda:0")
        t[aoff:aoff + s.size] = torch.from_numpy(s)
        return t, (t.data_ptr() + aoff, shape, count)
    off = np.ascontiguousarray(shape, dtype=np.uint64)
    count = off.size - 1
    if packed:
        words = rb.pack_batch(s, off, seed=k)
        w, woff, doff = _dev(np.concatenate([words, np.zeros(1, dtype=np.uint64)])), _dev(rb.word_offsets_of(off)), _dev(off)
        return (w, woff, doff), (w, woff, doff, count, words.size)
    t = torch.zeros(s.size + aoff + 16, dtype=torch.uint8, device="cuda:0")
    t[aoff:aoff + s.size] = torch.from_numpy(s)
    doff = _dev(off)
    return (t, doff), (t.data_ptr() + aoff, doff, count, s.size)


def _async_form(c, layout, packed, pattern):
    """the per-read _async method of (layout, packed, pattern)"""
    return {("fixed", False, False): c.reads_edist_start_async, ("fixed", True, False): c.reads_edist_start_packed_async,
            ("fixed", False, True): c.reads_pattern_edist_start_async, ("fixed", True, True): c.reads_pattern_edist_start_packed_async,
            ("ragged", False, False): c.reads_edist_start_batch_async, ("ragged", True, False): c.reads_edist_start_batch_packed_async,
            ("ragged", False, True): c.reads_pattern_edist_start_batch_async,
            ("ragged", True, True): c.reads_pattern_edist_start_batch_packed_async}[(layout, packed, pattern)]


def _host_form(c, layout, packed, pattern):
    return {("fixed", False, False): c.reads_edist_start, ("fixed", True, False): c.reads_edist_start_packed,
            ("fixed", False, True): c.reads_pattern_edist_start, ("fixed", True, True): c.reads_pattern_edist_start_packed,
            ("ragged", False, False): c.reads_edist_start_batch, ("ragged", True, False): c.reads_edist_start_batch_packed,
            ("ragged", False, True): c.reads_pattern_edist_start_batch,
            ("ragged", True, True): c.reads_pattern_edist_start_batch_packed}[(layout, packed, pattern)]


def _ref_forms(c, free, packed, pattern):
    """(the _async method, the host method) along a reference"""
    return {(False, False): (c.kmer_edist_start_async, free.kmer_edist_start), (True, False): (c.kmer_edist_start_packed_async, free.kmer_edist_start_packed),
            (False, True): (c.kmer_pattern_edist_start_async, free.kmer_pattern_edist_start),
            (True, True): (c.kmer_pattern_edist_start_packed_async, free.kmer_pattern_edist_start_packed)}[(packed, pattern)]


def dev_reads(ctx, layout, packed, pattern, s, shape, k, anchor, pos, queries, query, end, aoff=0):
    keep, head = _reads_data(layout, packed, s, shape, k, aoff)
    q = _dev_queries(queries, pattern)
    o = Out(len(query))
    _async_form(ctx, layout, packed, pattern)(*head, k, q, len(queries), _dev(np.asarray(query, dtype=np.uint32)), _dev(np.asarray(end, dtype=np.uint32)),
                                                             *o.ptrs(), "end" if anchor else "start", pos)
    return o.read(ctx)


def host_reads(layout, packed, pattern, s, shape, k, anchor, pos, queries, query, end, ctx=None):
    from bitnuc_amd import api
    c = ctx or api.context_free()
    a = "end" if anchor else "start"
    fn = _host_form(c, layout, packed, pattern)
    if layout == "fixed":
        count = len(query)
        return fn(ro.pack_reads(s, shape, count), shape, count, k, queries, query, end, a, pos) if packed else fn(s, shape, k, queries, query, end, a, pos, count)
    off = np.ascontiguousarray(shape, dtype=np.uint64)
    if packed:
        return fn(rb.pack_batch(s, off, seed=k), rb.word_offsets_of(off), off, k, queries, query, end, a, pos)
    return fn(s, off, k, queries, query, end, a, pos)


def want_reads(s, off, k, anchor, pos, queries, query, end):
    codes = ro.codes_of(s)
    off = [int(x) for x in off]
    texts = [codes[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    floors = [so.floor_of(len(t), k, anchor, pos) for t in texts]
    start, dist = so.starts(texts, floors, so.masks_of(queries, k), k, query, end)
    return start.astype(np.uint32), dist


def _batch(rng, k, lens, queries, lower=0.3):
    """random reads that carry a copy of one of the queries (a third with one base deleted, a third with one inserted) where they can hold it"""
    off = rb.offsets_of(lens)
    s = _ascii(rng.integers(0, 4, size=int(off[-1])))
    for r, ln in enumerate(lens):
        c = [int(x) for x in ro.query_codes(queries[r % len(queries)], k)]
        if r % 3 == 0 and k >= 3:
            del c[k // 2]
        elif r % 3 == 1 and k >= 2:
            c.insert(k // 2, next(x for x in range(4) if x != c[k // 2 - 1] and x != c[k // 2]))
        if ln >= len(c):
            at = int(off[r]) + int(rng.integers(0, ln - len(c) + 1))
            s[at:at + len(c)] = _ascii(c)
    s[rng.random(s.size) < lower] |= 0x20
    return s, off


def check(ctx, layouts, s, off, k, anchor, pos, queries, query, end, aoffs=(0,), fixed_len=None):
    """oracle == host form == device form, for every form that can hold the batch"""
    want = want_reads(s, off, k, anchor, pos, queries, query, end)
    pats = rp.singletons(queries, k)
    for layout in layouts:
        shape = fixed_len if layout == "fixed" else off
        for packed in (False, True):
            for pattern in (False, True):
                qs = pats if pattern else queries
                host = host_reads(layout, packed, pattern, s, shape, k, anchor, pos, qs, query, end)
                assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]), ("host", layout, packed, pattern)
                for aoff in ((0,) if packed else aoffs):
                    got = dev_reads(ctx, layout, packed, pattern, s, shape, k, anchor, pos, qs, query, end, aoff)
                    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
                    assert bad.size == 0, (layout, packed, pattern, aoff, int(bad[0]), int(got[0][bad[0]]), int(got[1][bad[0]]), int(want[0][bad[0]]), int(want[1][bad[0]]))
    return want


@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_333_reads_of_k_to_200_bases_ragged_and_fixed(ctx, k):
    rng = np.random.default_rng(0x333 + k)
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(5)], dtype=np.uint64)
    # ragged: lengths k .. 200; the ends anywhere from one in front of the floor to one behind the read; both anchors
    lens = rng.integers(k, 201, size=COUNT)
    s, off = _batch(rng, k, lens, queries)
    for anchor, pos in ((0, 0), (0, 7), (1, 0), (1, 9)):
        query = rng.integers(0, 6, size=COUNT).astype(np.uint32)  # 5: no such query
        floors = [so.floor_of(int(ln), k, anchor, pos) for ln in lens]
        end = np.array([max(0, int(rng.integers(min(f, int(ln)) - 1, max(int(ln), f) + 2))) for f, ln in zip(floors, lens)], dtype=np.uint32)
        check(ctx, ("ragged",), s, off, k, anchor, pos, queries, query, end, aoffs=(0, 1, 2, 3))
    # fixed: 150 bases
    L = 150
    s, off = _batch(rng, k, [L] * COUNT, queries)
    for anchor, pos in ((0, 0), (0, 11), (1, 4)):
        query = rng.integers(0, 6, size=COUNT).astype(np.uint32)
        end = rng.integers(0, L + 2, size=COUNT).astype(np.uint32)
        check(ctx, ("fixed", "ragged"), s, off, k, anchor, pos, queries, query, end, aoffs=(0, 3), fixed_len=L)


def test_window_placement_in_dwords_and_words(ctx):
    """k = 32: w = 63.  ASCII: the window's first byte at every byte of a dword (buffer offsets 0 .. 3 x ends 63 .. 70), so that it spans 16 or 17 dwords;
    packed: ends at 0, 1 and 31 mod 32 with windows of 1 .. 63 bases: one, two and three words"""
    rng = np.random.default_rng(0x91ACE)
    k = 32
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(2)], dtype=np.uint64)
    L = 200
    ends = [63, 64, 65, 66, 67, 70, 95, 96, 97, 127, 128, 129, 159, 160, 161, 200, 31, 32, 33, 1, 0, 62]
    count = len(ends) * 3
    s, off = _batch(rng, k, [L] * count, queries)
    end = np.array([ends[r % len(ends)] for r in range(count)], dtype=np.uint32)
    query = (np.arange(count) % 2).astype(np.uint32)
    check(ctx, ("fixed", "ragged"), s, off, k, 0, 0, queries, query, end, aoffs=(0, 1, 2, 3), fixed_len=L)
    for pos in (30, 31, 33, 60, 64, 96, 120):  # the floor cuts the window: 1 .. 63 bases in one, two or three words
        check(ctx, ("fixed", "ragged"), s, off, k, 0, pos, queries, query, end, aoffs=(1,), fixed_len=L)


def test_waves_of_equal_w_of_mixed_w_and_of_skipped_items(ctx):
    rng = np.random.default_rng(0x3A7E5)
    k = 16
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(3)], dtype=np.uint64)
    L = 100
    count = 64 * 5 + 13
    s, off = _batch(rng, k, [L] * count, queries)
    query = (np.arange(count) % 3).astype(np.uint32)
    end = np.zeros(count, dtype=np.uint32)
    end[0:64] = 80                      # a wave of equal w = 31
    end[64:128] = np.arange(64) % 40    # mixed w: 0 .. 31, several lanes with w = 0
    query[128:192] = 3                  # a wave of skipped items: no such query ...
    end[128:192] = 50
    end[192:256] = 0                    # a wave of w = 0: the empty substring everywhere
    end[256:320] = L + 1 + np.arange(64)  # ... and ends behind the read
    end[320:] = 7                       # the partial last wave, w = 7
    want = check(ctx, ("fixed", "ragged"), s, off, k, 0, 0, queries, query, end, aoffs=(0, 2), fixed_len=L)
    assert (want[0][128:192] == 0xFFFFFFFF).all() and (want[1][192:256] == k).all() and (want[0][192:256] == 0).all()


def _forward_forms(ctx, k, queries, s, off, fixed_len, pattern, packed):
    """(name, forward call(outs) , (anchor, pos)) of the forward _async forms of one (query kind, input kind): whole read and anchored, fixed and ragged"""
    import torch
    count = len(off) - 1
    qs = rp.singletons(queries, k) if pattern else queries
    dq = _dev_queries(qs, pattern)
    pre = "reads_pattern_edist_" if pattern else "reads_edist_"
    sfx = ("_packed" if packed else "") + "_async"
    keep_f, head_f = _reads_data("fixed", packed, s, fixed_len, k)
    keep_r, head_r = _reads_data("ragged", packed, s, off, k)
    span = min(20, 63 - k)
    forms = [
        ("fixed", head_f, lambda o: getattr(ctx, pre + "best" + sfx)(*head_f, k, dq, len(queries), *o), (0, 0)),
        ("fixed", head_f, lambda o: getattr(ctx, pre + "anchored" + sfx)(*head_f, k, dq, len(queries), *o, pos_lo=3, pos_hi=3 + span), (0, 3)),
        ("ragged", head_r, lambda o: getattr(ctx, pre + "best_batch" + sfx)(*head_r, k, dq, len(queries), *o), (0, 0)),
        ("ragged", head_r, lambda o: getattr(ctx, pre + "anchored_batch" + sfx)(*head_r, k, dq, len(queries), *o, pos_lo=2, pos_hi=2 + span, anchor="start"), (0, 2)),
        ("ragged", head_r, lambda o: getattr(ctx, pre + "anchored_batch" + sfx)(*head_r, k, dq, len(queries), *o, pos_lo=0, pos_hi=span, anchor="end"), (1, span)),
    ]
    return forms, dq, (keep_f, keep_r), count, torch


@pytest.mark.parametrize("k", [16, 31])
def test_every_forward_async_per_read_form_followed_by_the_start_form(ctx, k):
    import torch
    rng = np.random.default_rng(0xF0A + k)
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(4)], dtype=np.uint64)
    L = 2 * k + 40
    s, off = _batch(rng, k, [L] * COUNT, queries, lower=0.0)
    codes = ro.codes_of(s)
    texts = [codes[r * L:(r + 1) * L] for r in range(COUNT)]
    seen = set()
    for pattern in (False, True):
        for packed in (False, True):
            forms, dq, keep, count, _ = _forward_forms(ctx, k, queries, s, off, L, pattern, packed)
            qs = rp.singletons(queries, k) if pattern else queries
            for layout, head, forward, (anchor, pos) in forms:
                fw = [torch.full((count,), 0x5A, dtype=t, device="cuda:0") for t in (torch.int32, torch.int32, torch.uint8) * 2]
                forward(fw)
                outs = []
                for j in (0, 1):  # the start call chained behind the forward call, no sync between them: best, then the runner-up
                    o = Out(count)
                    _async_form(ctx, layout, packed, pattern)(*head, k, dq, len(queries), fw[3 * j], fw[3 * j + 1], *o.ptrs(), "end" if anchor else "start", pos)
                    outs.append(o)
                for j, o in enumerate(outs):
                    start, dist = o.read(ctx)
                    fq, fe, fd = (fw[3 * j + i].cpu().numpy().view((np.uint32, np.uint32, np.uint8)[i]) for i in range(3))
                    live = fq != 0xFFFFFFFF
                    assert live.any() and np.array_equal(dist, fd), (layout, pattern, packed, j)  # the forward dist on ALL items (fills are fills)
                    hs, hd = host_reads(layout, packed, pattern, s, L if layout == "fixed" else off, k, anchor, pos, qs, fq, fe)
                    assert np.array_equal(start, hs) and np.array_equal(dist, hd) and (start[live] <= fe[live]).all()  # the host form on all items ...
                    m = 70  # ... and the oracle on the first ones (more than a wave)
                    ws, wd = so.starts(texts[:m], [so.floor_of(L, k, anchor, pos)] * m, so.masks_of(queries, k), k, fq[:m], fe[:m])
                    assert np.array_equal(start[:m], ws.astype(np.uint32)) and np.array_equal(dist[:m], wd)
                seen.add((layout, pattern, packed, anchor, pos))
    assert len(seen) == 20  # the 16 forward forms, the four ragged anchored ones under both anchors


def _hits_async(ctx, pattern, packed):
    return getattr(ctx, "kmer_" + ("pattern_" if pattern else "") + "edist_hits" + ("_packed" if packed else "") + "_async")


@pytest.mark.parametrize("k", [16, 31])
def test_reference_forms_best_and_hit_lists_through_the_device_count(ctx, k):
    """the 12 forward forms along a reference (best: 4; hits with the cap above and below *n_hits: 4 + 4), each followed by the start call; the hit list
    feeds it through d_n_hits: entries at and beyond min(m, *d_m) are untouched"""
    import torch
    from bitnuc_amd import api
    free = api.context_free()
    rng = np.random.default_rng(0x4EF + k)
    Q = 3
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(Q)], dtype=np.uint64)
    pats = rp.singletons(queries, k)
    n = 20_011
    ref = _ascii(rng.integers(0, 4, size=n))
    for i, at in enumerate((1000, 9000, 15000, 19000)):
        c = [int(x) for x in ro.query_codes(queries[i % Q], k)]
        if i % 2:
            del c[k // 2]
        ref[at:at + len(c)] = _ascii(c)
    rc = ro.codes_of(ref)
    w = ro.pack_reads(ref, n, 1)
    d_ref, d_w = _dev(np.concatenate([ref, np.zeros(8, dtype=np.uint8)])), _dev(w)
    seen = 0
    for pattern in (False, True):
        qs = pats if pattern else queries
        dq = _dev_queries(qs, pattern)
        pre = "kmer_pattern_edist_" if pattern else "kmer_edist_"
        for packed in (False, True):
            head = (d_w, w.size, n) if packed else (d_ref, n)
            sfx = "_packed" if packed else ""
            start_async, start_host = _ref_forms(ctx, free, packed, pattern)
            # best: one item per query
            d_end = torch.zeros(Q, dtype=torch.int64, device="cuda:0")
            d_dist = torch.zeros(Q, dtype=torch.uint8, device="cuda:0")
            getattr(ctx, pre + "best" + sfx + "_async")(*head, k, dq, Q, d_end, d_dist)
            o = Out(Q, wide=True)
            start_async(*head, k, dq, Q, _dev(np.arange(Q, dtype=np.uint32)), d_end, Q, *o.ptrs())
            start, dist = o.read(ctx)
            end = d_end.cpu().numpy().view(np.uint64)
            ws, wd = so.starts([rc] * Q, [0] * Q, so.masks_of(queries, k), k, np.arange(Q), end, fill=so.FILL64)
            assert np.array_equal(start, ws) and np.array_equal(dist, wd) and np.array_equal(dist, d_dist.cpu().numpy())
            hs, hd = start_host(*((w, n) if packed else (ref,)), k, qs, end, np.arange(Q, dtype=np.uint32))
            assert np.array_equal(hs, ws) and np.array_equal(hd, wd)
            seen += 1
            # hits of query 1 at tau = 2, the cap above and below the number of hits
            one = qs[1] if pattern else int(queries[1])
            total = int(getattr(free, pre + "hits" + sfx)(*((w, n) if packed else (ref,)), k, one, 2).size)
            assert total >= 3
            for cap in (total + 5, total - 2):
                d_e = torch.full((cap,), -1, dtype=torch.int64, device="cuda:0")
                d_hd = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
                d_n = torch.zeros(1, dtype=torch.int64, device="cuda:0")
                _hits_async(ctx, pattern, packed)(*head, k, one, 2, d_e, d_hd, cap, d_n)
                o = Out(cap, wide=True)
                start_async(*head, k, dq[1:2], 1, None, d_e, cap, *o.ptrs(), d_m=d_n)
                m = min(cap, total)
                start, dist = o.read(ctx, written=m)
                assert int(d_n.item()) == total
                ends = d_e.cpu().numpy().view(np.uint64)[:m]
                ws, wd = so.starts([rc] * m, [0] * m, so.masks_of(queries[1:2], k), k, np.zeros(m, dtype=np.int64), ends, fill=so.FILL64)
                assert np.array_equal(start, ws) and np.array_equal(dist, wd) and np.array_equal(dist, d_hd.cpu().numpy()[:m]) and (start <= ends).all()
                seen += 1
    assert seen == 12


def test_queue_forward_start_forward_start_with_one_sync(ctx):
    """forward (17 queries) -> start -> forward (5 queries) -> start on one context without a sync in between: the table slot both calls use is safe by
    stream order alone"""
    import torch
    rng = np.random.default_rng(0x9E0E)
    k, L = 16, 120
    jobs = []
    for nq in (17, 5):
        queries = ro.random_queries(rng, nq, k)
        s, off = _batch(rng, k, [L] * COUNT, queries)
        keep, head = _reads_data("fixed", False, s, L, k, 1)
        dq = _dev_queries(queries, False)
        fw = [torch.zeros(COUNT, dtype=t, device="cuda:0") for t in (torch.int32, torch.int32, torch.uint8)]
        jobs.append((queries, s, off, keep, head, dq, fw, Out(COUNT)))
    torch.cuda.synchronize()
    for queries, s, off, keep, head, dq, fw, o in jobs:
        ctx.reads_edist_best_async(*head, k, dq, len(queries), *fw)
        ctx.reads_edist_start_async(*head, k, dq, len(queries), fw[0], fw[1], *o.ptrs())
    ctx.sync()
    for queries, s, off, keep, head, dq, fw, o in jobs:
        start, dist = o.read(ctx)
        fq, fe, fd = fw[0].cpu().numpy().view(np.uint32), fw[1].cpu().numpy().view(np.uint32), fw[2].cpu().numpy()
        want = want_reads(s, off, k, 0, 0, queries, fq, fe)
        assert np.array_equal(start, want[0]) and np.array_equal(dist, want[1]) and np.array_equal(dist, fd)


def test_graph_of_forward_and_start_replayed_on_new_reads():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(0x62A9)
    k, L, nq = 31, 150, 6
    queries = ro.random_queries(rng, nq, k)
    s1, off = _batch(rng, k, [L] * COUNT, queries)
    s2, _ = _batch(rng, k, [L] * COUNT, queries)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, head = _reads_data("fixed", False, s1, L, k, 3)
        dq = _dev_queries(queries, False)
        fw = [torch.zeros(COUNT, dtype=x, device="cuda:0") for x in (torch.int32, torch.int32, torch.uint8)]
        o = Out(COUNT)

        def run():
            c.reads_edist_best_async(*head, k, dq, nq, *fw)
            c.reads_edist_start_async(*head, k, dq, nq, fw[0], fw[1], *o.ptrs())
        run()  # the warm-up sizes the scratch
        start, dist = o.read(c)
        want = want_reads(s1, off, k, 0, 0, queries, fw[0].cpu().numpy().view(np.uint32), fw[1].cpu().numpy().view(np.uint32))
        assert np.array_equal(start, want[0]) and np.array_equal(dist, want[1])
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                run()
            t[3:3 + s2.size] = torch.from_numpy(s2).to(t.device)
            o.s.fill_(MARK32), o.d.fill_(0x5A)
            g.replay()
            start, dist = o.read(c)
            fq, fe, fd = fw[0].cpu().numpy().view(np.uint32), fw[1].cpu().numpy().view(np.uint32), fw[2].cpu().numpy()
            want = want_reads(s2, off, k, 0, 0, queries, fq, fe)
            assert np.array_equal(start, want[0]) and np.array_equal(dist, want[1]) and np.array_equal(dist, fd)
            assert not np.array_equal(s1, s2)
        finally:
            g.reset()
            del g
            c.close()


def test_an_invalid_byte_in_a_walked_range_is_reported_once(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(0x1BAD)
    k, L = 16, 90
    queries = ro.random_queries(rng, 2, k)
    s, off = _batch(rng, k, [L] * COUNT, queries)
    query = np.zeros(COUNT, dtype=np.uint32)
    end = np.full(COUNT, 60, dtype=np.uint32)  # the walked range of read r: its bytes [29, 60)
    for layout, shape in (("fixed", L), ("ragged", off)):
        for at, later, reported in ((200 * L + 29, 250 * L + 40, True), (7 * L + 59, None, True), (9 * L + 28, None, False), (9 * L + 60, None, False)):
            c = s.copy()
            c[at] = ord("N")
            if later is not None:
                c[later] = ord("x")  # the first in buffer order wins
            keep, head = _reads_data(layout, False, c, shape, k, 2)
            o = Out(COUNT)
            torch.cuda.synchronize()
            _async_form(ctx, layout, False, False)(*head, k, _dev_queries(queries, False), 2, _dev(query), _dev(end), *o.ptrs())
            if reported:
                with pytest.raises(bn.NucleotideError) as ei:
                    ctx.sync()
                assert (ei.value.byte, ei.value.index) == (ord("N"), at)
                del ei
            ctx.sync()  # latched once: nothing is left for the next sync; a byte beside the walked range is never examined
    # along a reference
    n = 4000
    ref = _ascii(rng.integers(0, 4, size=n))
    ref[1234] = ord("N")
    ends = np.array([3000, 1234 + 31, 1234, 1235], dtype=np.uint64)  # 1234 + 31: the window's first byte; 1234: right behind a window
    for sel, reported in (((0, 2), False), ((0, 1), True), ((3,), True)):
        o = Out(len(sel), wide=True)
        torch.cuda.synchronize()
        ctx.kmer_edist_start_async(_dev(ref), n, k, _dev_queries(queries, False), 2, None, _dev(ends[list(sel)]), len(sel), *o.ptrs())
        if reported:
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (ord("N"), 1234)
            del ei
        ctx.sync()


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two(ctx):
    """one chunk: the session context sends every host form to the device (force_gpu).  Two chunks: 900,000 reads of 150 bases (the ASCII forms cut at
    128 Mi bytes, the packed ones at 4 Mi words) on a context with the default dispatch; the oracle runs on the reads around the boundaries, the first and
    the last ones, everywhere else the result must equal the _async form's on the whole batch.  Then an N past the boundary reports its absolute index."""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(0xC4A2)
    k, L = 16, 150
    queries = ro.random_queries(rng, 3, k)
    s, off = _batch(rng, k, list(rng.integers(0, 201, size=COUNT)), queries)
    lens = np.diff(off.astype(np.int64))
    query = rng.integers(0, 4, size=COUNT).astype(np.uint32)
    end = np.array([int(rng.integers(0, ln + 2)) for ln in lens], dtype=np.uint32)
    want = want_reads(s, off, k, 1, 3, queries, query, end)
    for packed in (False, True):
        for pattern in (False, True):
            got = host_reads("ragged", packed, pattern, s, off, k, 1, 3, rp.singletons(queries, k) if pattern else queries, query, end, ctx=ctx)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    count = 900_000
    per_ascii, per_packed = (128 << 20) // L, ((128 << 20) // 32) // 5
    codes = rng.integers(0, 4, size=count * L, dtype=np.uint8)
    qc = ro.query_codes(queries[0], k)
    for per in (per_ascii, per_packed):
        codes[per * L - k:per * L] = qc
        codes[per * L + 40:per * L + 40 + k - 1] = np.delete(qc, 5)
    big = ro.LUT[codes]
    query = (np.arange(count) % 3).astype(np.uint32)
    end = rng.integers(0, L + 1, size=count).astype(np.uint32)
    for per in (per_ascii, per_packed):
        query[per - 1:per + 1] = 0
        end[per - 1], end[per] = L, 40 + k - 1
    rows = np.unique(np.concatenate([np.arange(100), np.arange(count - 100, count)] + [np.arange(per - 50, per + 50) for per in (per_ascii, per_packed)]))
    sample = np.ascontiguousarray(big.reshape(count, L)[rows]).reshape(-1)
    ws, wd = want_reads(sample, np.arange(rows.size + 1) * L, k, 0, 0, queries, query[rows], end[rows])
    c = bn.Context(0)
    try:
        keep, head = _reads_data("fixed", False, big, L, k)
        o = Out(count)
        c.reads_edist_start_async(*head, k, _dev_queries(queries, False), 3, _dev(query), _dev(end), *o.ptrs())
        dev = o.read(c)
        del keep, o
        assert np.array_equal(dev[0][rows], ws) and np.array_equal(dev[1][rows], wd)
        for per in (per_ascii, per_packed):
            at = int(np.searchsorted(rows, per))
            assert (int(ws[at - 1]), int(wd[at - 1])) == (L - k, 0) and int(wd[at]) == 1
        bigoff = np.arange(count + 1, dtype=np.uint64) * L
        words = ro.pack_reads(big, L, count)
        for got in (c.reads_edist_start(big, L, k, queries, query, end), c.reads_edist_start_packed(words, L, count, k, queries, query, end),
                    c.reads_edist_start_batch(big, bigoff, k, queries, query, end),
                    c.reads_pattern_edist_start_batch_packed(words, rb.word_offsets_of(bigoff), bigoff, k, rp.singletons(queries, k), query, end)):
            assert np.array_equal(got[0], dev[0]) and np.array_equal(got[1], dev[1])
        at = (per_ascii + 7) * L + 33
        big[at] = ord("N")
        end[per_ascii + 7] = 40
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_edist_start(big, L, k, queries, query, end)
        assert (ei.value.byte, ei.value.index) == (ord("N"), at)
        del ei
    finally:
        c.close()


def test_references_of_more_than_2_to_the_32_bases(ctx):
    """two references of 2^32 + 4096 bases, both A-filled on the device: packed (1 GiB of words) and ASCII; copies of the query (one with a deleted base)
    planted at ends just below, across and above 2^32; items only there and at the buffer's first and last base"""
    import torch
    k = 31
    n = (1 << 32) + 4096
    rng = np.random.default_rng(0x2327)
    qc = np.array([1, 2, 3] * 10 + [1])  # no A: the fill matches nowhere
    queries = np.array([ro.word_of(qc)], dtype=np.uint64)
    short = np.delete(qc, 15)
    plants = [((1 << 32) - 100 - k, qc), ((1 << 32) - 12, qc), ((1 << 32) + 50, short), (n - k, qc)]
    ends = np.array([0, 1, 40] + [at + len(c) for at, c in plants] + [(1 << 32) + 50 + 29, (1 << 32), n - 1, n, n + 1], dtype=np.uint64)
    # the oracle on the 70 bases in front of each end
    ws, wd = np.zeros(ends.size, dtype=np.uint64), np.zeros(ends.size, dtype=np.uint8)
    for i, e in enumerate(int(x) for x in ends):
        if e > n:
            ws[i], wd[i] = so.FILL64, 0xFF
            continue
        lo = max(0, e - 70)
        local = np.zeros(e - lo, dtype=np.int64)
        for at, c in plants:
            for j, x in enumerate(c):
                if lo <= at + j < e:
                    local[at + j - lo] = x
        a, b = so.starts([local], [0], so.masks_of(queries, k), k, [0], [e - lo], fill=so.FILL64)
        ws[i], wd[i] = int(a[0]) + lo, b[0]
    assert [int(x) for x in wd[3:7]] == [0, 0, 1, 0] and int(ws[4]) == (1 << 32) - 12 and int(ws[5]) == (1 << 32) + 50
    dq = _dev_queries(queries, False)
    # packed: A is code 0
    words = torch.zeros((n + 31) // 32, dtype=torch.int64, device="cuda:0")
    for at, c in plants:
        w0, w1 = at // 32, (at + len(c) + 31) // 32
        bits = np.zeros((w1 - w0) * 32, dtype=np.uint64)
        bits[at - 32 * w0:at - 32 * w0 + len(c)] = c
        words[w0:w1] = _dev(np.bitwise_or.reduce(bits.reshape(-1, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1))
    o = Out(ends.size, wide=True)
    ctx.kmer_edist_start_packed_async(words, words.numel(), n, k, dq, 1, None, _dev(ends), ends.size, *o.ptrs())
    start, dist = o.read(ctx)
    assert np.array_equal(start, ws) and np.array_equal(dist, wd)
    del words
    ref = torch.full((n + 16,), ord("A"), dtype=torch.uint8, device="cuda:0")
    for at, c in plants:
        ref[at:at + len(c)] = _dev(_ascii(c))
    o = Out(ends.size, wide=True)
    ctx.kmer_edist_start_async(ref, n, k, dq, 1, None, _dev(ends), ends.size, *o.ptrs())
    start, dist = o.read(ctx)
    assert np.array_equal(start, ws) and np.array_equal(dist, wd)
    del ref
    torch.cuda.empty_cache()
