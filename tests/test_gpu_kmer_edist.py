"""GPU tests of the indel-tolerant k-mer search along a reference (bitnuc_kmer_edist_best*, bitnuc_kmer_edist_count_multi* and their pattern twins;
scan_edist_ref_device.h) against tests/kmer_edist_oracle.py, the plain DP: every comparison is exact equality.

Sizes around the kernel's boundaries (C = the chunk of end positions a lane owns): 1, k, C - 1, C, C + 1, C + 2k - 1, C + 2k, C + 2k + 1, 64 C +- 1 (a
wave), 256 C +- 1 (a workgroup) and 10^6 + 7; k in {1, 2, 15, 16, 17, 31, 32}; Q in {1, 2, 3, 4, 5, 7, 9, 33} (the interleave of four and its remainders
of two and one); ASCII at byte offsets +0 / +1 / +7 / +15 with about 30 % lowercase, packed words at 16-byte and 8-mod-16 offsets.
THE SEAM is the only new way to be wrong: a copy of the query with d inserted bases that ends e bases behind the start of a chunk, of a wave's and of a
workgroup's first chunk, for which the test first shows ON THE ORACLE that a walk starting k + d - 1 bases before that end would report a larger value
(so a kernel whose lead-in is too short fails); exact copies at the same places; equal distances in two chunks (the leftmost end wins); the count, in
which a column reported twice or never shows.  Guard words and bytes around the outputs, the fill without windows, invalid bytes (first, last, in a
chunk's lead-in; the smallest index of two), a hipGraph replay after the reference and the queries changed, a queue mixed with Hamming calls and one
sync, the host-pointer forms above the cutoff in one chunk and across two, one packed case past 2^32 bases (which also crosses the grid's wrap: a round
of the bounded grid covers 2^29 bases), and the bitnuc.hpp mirror."""
import numpy as np
import pytest

import kmer_edist_oracle as ko
import pattern_oracle as po

pytestmark = pytest.mark.gpu

C = 1024   # kEdistRefChunk in bitnuc_amd/csrc/scan_edist_ref_device.h: the end positions one lane owns per round (its header comment has the rule)
WAVE = 64 * C
GROUP = 256 * C  # kEdistRefBlock lanes
KS = (1, 2, 15, 16, 17, 31, 32)
QS = (1, 2, 3, 4, 5, 7, 9, 33)
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
NO_END = np.uint64(2**64 - 1)
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _ascii(codes, rng=None):
    s = LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)
    if rng is not None:
        s[rng.random(s.size) < 0.3] |= 0x20  # about 30 % lowercase
    return s


def _queries(rng, nq, k):
    """random queries with junk above 2k"""
    return rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=nq, dtype=np.uint64)


def _qcodes(q, k):
    return np.array([(int(q) >> (2 * b)) & 3 for b in range(k)], dtype=np.int64)


def _word(codes):
    return sum(int(c) << (2 * b) for b, c in enumerate(codes))


def _with_insert(rng, qc, d):
    """the query's codes with d random bases inserted after position k / 2"""
    h = len(qc) // 2
    return np.concatenate([qc[:h], rng.integers(0, 4, size=d), qc[h:]])


def _text(rng, n, k, queries):
    """n random codes with edited copies of the first queries planted where they fit"""
    codes = rng.integers(0, 4, size=n)
    for i, q in enumerate(queries[:6]):
        c = _qcodes(q, k)
        if i % 3 == 1 and k > 2:
            c = np.delete(c, int(rng.integers(0, k)))
        elif i % 3 == 2:
            c = np.insert(c, int(rng.integers(0, k)), int(rng.integers(0, 4)))
        if len(c) <= n:
            p = int(rng.integers(0, n - len(c) + 1))
            codes[p:p + len(c)] = c
    return codes


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).to("cuda:0")


def _dev_queries(queries, pattern):
    return _dev(ko.as_patterns(queries), np.int32) if pattern else _dev(np.asarray(queries, dtype=np.uint64), np.int64)


def _outputs(nq, dist_off=1):
    """end / counts with guard words after [nq]; dist inside a guarded buffer, starting at byte dist_off of it"""
    import torch
    end = torch.full((nq + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    dbuf = torch.full((dist_off + nq + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    return end, dbuf, dbuf.data_ptr() + dist_off


def _read(ctx, end, dbuf, nq, dist_off=1):
    ctx.sync()
    p = end.cpu().numpy().view(np.uint64)
    d = dbuf.cpu().numpy()
    assert (p[nq:] == np.uint64(FILL)).all(), "end / counts written after n_queries"
    assert (d[:dist_off] == 0x5A).all() and (d[dist_off + nq:] == 0x5A).all(), "dist written outside [0, n_queries)"
    return p[:nq].copy(), d[dist_off:dist_off + nq].copy()


def _ascii_dev(s, off):
    import torch
    t = torch.full((s.size + off + 16,), ord("N"), dtype=torch.uint8, device="cuda:0")  # an N on either side: a byte read outside [0, n) is an error
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    return t, t.data_ptr() + off


def _words_dev(w, off):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    return t, t.data_ptr() + 8 * off


def _device_forms(ctx):
    """(best, count) of the eight asynchronous forms by (pattern queries?, layout)"""
    return {(False, "ascii"): (ctx.kmer_edist_best_async, ctx.kmer_edist_count_multi_async),
            (False, "packed"): (ctx.kmer_edist_best_packed_async, ctx.kmer_edist_count_multi_packed_async),
            (True, "ascii"): (ctx.kmer_pattern_edist_best_async, ctx.kmer_pattern_edist_count_multi_async),
            (True, "packed"): (ctx.kmer_pattern_edist_best_packed_async, ctx.kmer_pattern_edist_count_multi_packed_async)}


def _run(ctx, codes, k, queries, taus, off=0, woff=0, pattern=False, rng=None, forms=("ascii", "packed")):
    """{form: (end, dist, counts)} of the device forms, guards checked; queries: exact words, or (Q, 4) patterns with pattern=True"""
    import torch
    n = len(codes)
    nq = len(queries)
    dq = _dev_queries(queries, pattern)
    dt = _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(taus, dtype=np.uint32), (nq,))), np.int32)
    out = {}
    keep = []
    for form in forms:
        e, db, dp = _outputs(nq)
        c, cb, _ = _outputs(nq)
        if form == "ascii":
            t, ptr = _ascii_dev(_ascii(codes, rng), off)
            head = (ptr, n, k)
        else:
            w = po.pack_codes(codes, junk=0xDEADBEEFCAFEF00D)
            t, ptr = _words_dev(w, woff)
            assert ptr % 16 == 8 * woff
            head = (ptr, w.size, n, k)
        keep.append(t)
        torch.cuda.synchronize()
        best, count = _device_forms(ctx)[(pattern, form)]
        best(*head, dq, nq, e, dp)
        count(*head, dq, dt, nq, c)
        end, dist = _read(ctx, e, db, nq)
        cnt, untouched = _read(ctx, c, cb, nq)
        assert (untouched == 0x5A).all()
        out[form] = (end, dist, cnt)
    return out


def _check(got, want, what):
    for form, g in got.items():
        for name, a, b in zip(("end", "dist", "counts"), g, want):
            assert np.array_equal(a, np.asarray(b, dtype=a.dtype)), (what, form, name, list(a[:6]), list(np.asarray(b)[:6]))


def _sizes(k):
    return sorted({1, k, C - 1, C, C + 1, C + 2 * k - 1, C + 2 * k, C + 2 * k + 1, WAVE - 1, WAVE + 1, GROUP - 1, GROUP + 1})


# ---- 1. sizes, k, Q and alignments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_sizes_around_the_chunk_the_wave_and_the_workgroup(ctx, k):
    rng = np.random.default_rng(9100 + k)
    for si, n in enumerate(_sizes(k)):
        if n < k:
            continue
        nq = QS[(si + k) % len(QS)] if n <= 2 * C + 100 else (1, 2, 3, 5)[(si + k) % 4]  # the DP oracle is O(n k Q): few queries at the large sizes
        pattern = (si + k) % 3 == 0
        queries = _queries(rng, nq, k)
        codes = _text(rng, n, k, queries)
        pats = ko.singletons(queries, k)
        if pattern:  # random sets, an all-N and an empty position among them
            pats = ko.as_patterns([po.from_sets(po.random_sets(rng, k)) if q % 2 else pats[q] for q in range(nq)])
        taus = rng.integers(0, k + 1, size=nq)
        want = ko.kmer_edist_both(codes, k, pats, taus)
        got = _run(ctx, codes, k, pats if pattern else queries, taus, off=(0, 1, 7, 15)[(si + k) % 4], woff=(si + k // 4) % 2, pattern=pattern, rng=rng)
        _check(got, want, (k, n, nq, pattern))


@pytest.mark.parametrize("nq", QS)
def test_query_counts_at_one_size(ctx, nq):
    rng = np.random.default_rng(400 + nq)
    k, n = 16, 2 * C + 2 * 16 + 77
    queries = _queries(rng, nq, k)
    codes = _text(rng, n, k, queries)
    taus = rng.integers(0, 5, size=nq)
    want = ko.kmer_edist_both(codes, k, ko.singletons(queries, k), taus)
    _check(_run(ctx, codes, k, queries, taus, off=nq % 4, woff=nq % 2, rng=rng), want, nq)
    _check(_run(ctx, codes, k, ko.singletons(queries, k), taus, pattern=True), want, nq)  # singleton patterns: the exact forms' results


def test_a_million_bases(ctx):
    rng = np.random.default_rng(1_000_007)
    k, n, nq = 31, 10**6 + 7, 4
    queries = _queries(rng, nq, k)
    codes = _text(rng, n, k, queries)
    taus = np.array([0, 1, 3, 2**32 - 1], dtype=np.uint32)
    want = ko.kmer_edist_both(codes, k, ko.singletons(queries, k), taus)
    assert want[2][3] == n
    _check(_run(ctx, codes, k, queries, taus, off=7, woff=1, rng=rng), want, n)


# ---- 2. the seam ----------------------------------------------------------------------------------------------------------------------
def _seam_case(seed, k, d, end, n):
    """(codes, query) with a copy of the query, d bases inserted after position k / 2, whose last base is the end-th of the text, such that THE ORACLE
    on the text cut k + d - 1 bases before that end gives a larger value at that end than on the whole text (another seed is drawn until it does): a walk
    that starts fresh there, as a kernel with too short a lead-in would, reports a wrong column.  E(end) depends on the 2k bases before it only, so the
    condition is tested on slices."""
    for attempt in range(200):
        rng = np.random.default_rng(seed * 1000 + attempt)
        q = _queries(rng, 1, k)
        codes = rng.integers(0, 4, size=n)
        plant = _with_insert(rng, _qcodes(q[0], k), d)
        codes[end - (k + d):end] = plant
        p = ko.singletons(q, k)[0]
        full = ko.ends(codes[max(0, end - 4 * k):end], k, p)[-1]
        cut = ko.ends(codes[end - (k + d - 1):end], k, p)[-1]
        if cut > full:
            return codes, q, int(full)
    raise AssertionError("no seed gives a case that needs the lead-in")


@pytest.mark.parametrize("seam", [C, 5 * C, WAVE, GROUP], ids=["chunk", "chunk5", "wave", "workgroup"])
@pytest.mark.parametrize("k,d", [(16, 1), (16, 4), (31, 7)])
def test_a_planted_bulge_across_the_seam(ctx, k, d, seam):
    n = seam + 2 * k + 300
    for e in (1, 2, k, k + d - 1, k + d, 2 * k - 1, 2 * k, 2 * k + 1):
        codes, q, at_plant = _seam_case(seam + 100 * k + e, k, d, seam + e, n)
        assert at_plant <= d
        want = ko.kmer_edist_both(codes, k, ko.singletons(q, k), at_plant)
        got = _run(ctx, codes, k, q, at_plant, off=e % 4, woff=e % 2)
        _check(got, want, (k, d, seam, e))


@pytest.mark.parametrize("seam", [C, WAVE, GROUP], ids=["chunk", "wave", "workgroup"])
def test_exact_copies_ties_and_the_lead_in_at_the_seam(ctx, seam):
    """query 0: exact copies that end e bases behind the seam, one text per e (dist 0, counted once at tau = 0); query 1: the same edited copy in the chunk
    before the seam and in the one behind it -- the leftmost end wins; query 2: a copy wholly inside the lead-in of the seam's chunk, which the chunk
    before reports once (the count says so)"""
    rng = np.random.default_rng(seam + 17)
    k = 16
    n = seam + C + 300
    for e in (1, 2, k, 2 * k - 1, 2 * k, 2 * k + 1):
        queries = _queries(rng, 3, k)
        codes = rng.integers(0, 4, size=n)
        codes[seam + e - k:seam + e] = _qcodes(queries[0], k)
        near = _qcodes(queries[1], k)
        near[5] ^= 1
        codes[seam - 500:seam - 500 + k] = near
        codes[seam + 200:seam + 200 + k] = near
        codes[seam - 40:seam - 40 + k] = _qcodes(queries[2], k)  # ends at seam - 24: a column of the lead-in
        want = ko.kmer_edist_both(codes, k, ko.singletons(queries, k), [0, 1, 0])
        assert (int(want[0][0]), int(want[1][0])) == (seam + e, 0) and (int(want[0][1]), int(want[1][1])) == (seam - 500 + k, 1)
        assert (int(want[0][2]), int(want[1][2])) == (seam - 24, 0) and list(want[2]) == [1, 2, 1]
        _check(_run(ctx, codes, k, queries, [0, 1, 0], off=e % 4, woff=e % 2), want, (seam, e))


# ---- 3. outputs and errors ---------------------------------------------------------------------------------------------------------------
def test_fills_without_windows(ctx):
    import torch
    codes = np.array([0, 1, 2, 3, 0, 1])
    for k, n in ((0, 6), (7, 6), (3, 0)):
        for pattern in (False, True):
            dq = _dev_queries(ko.singletons([1, 2, 3], 3) if pattern else [1, 2, 3], pattern)
            dt = _dev(np.array([9, 9, 9], dtype=np.uint32), np.int32)
            t, ptr = _ascii_dev(_ascii(codes[:n]), 1)
            tw, wptr = _words_dev(po.pack_codes(codes[:n]), 1)
            for form, head in (("ascii", (ptr, n, k)), ("packed", (wptr, (n + 31) // 32, n, k))):
                e, db, dp = _outputs(3)
                c, cb, _ = _outputs(3)
                torch.cuda.synchronize()
                best, count = _device_forms(ctx)[(pattern, form)]
                best(*head, dq, 3, e, dp)
                count(*head, dq, dt, 3, c)
                end, dist = _read(ctx, e, db, 3)
                assert (end == NO_END).all() and (dist == 0xFF).all()
                assert (_read(ctx, c, cb, 3)[0] == 0).all()


def test_invalid_bytes_are_latched_once_with_the_smallest_index(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(55)
    k, nq = 16, 5
    n = 3 * C + 77
    queries = _queries(rng, nq, k)
    codes = _text(rng, n, k, queries)
    s = _ascii(codes, rng)
    dq = _dev_queries(queries, False)
    dt = _dev(np.full(nq, 2, dtype=np.uint32), np.int32)
    for case, at in enumerate(((0,), (n - 1,), (C - 10,), (2 * C - 64,), (2 * C + 5, C + 3), (n - 1, 2 * C - 1))):  # C - 10, 2C - 64: in a chunk's lead-in
        b = s.copy()
        for i, a in enumerate(at):
            b[a] = (ord("N"), ord("x"))[i]
        first = min(at)
        for fn in ("best", "count_multi"):
            t, ptr = _ascii_dev(b, (0, 1, 7, 15)[case % 4])
            e, db, dp = _outputs(nq)
            torch.cuda.synchronize()
            if fn == "best":
                ctx.kmer_edist_best_async(ptr, n, k, dq, nq, e, dp)
            else:
                ctx.kmer_edist_count_multi_async(ptr, n, k, dq, dt, nq, e)
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (int(b[first]), first), (case, fn)
            del ei
            ctx.sync()  # latched once: nothing left for the next sync
    _check(_run(ctx, codes, k, queries, 2, rng=rng), ko.kmer_edist_both(codes, k, ko.singletons(queries, k), 2), "clean after the errors")


# ---- 4. graphs and queues -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reference_and_the_queries_changed():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    n, k, nq = 70_001, 23, 7
    q1, q2 = _queries(rng, nq, k), _queries(rng, nq, k)
    c1, c2 = _text(rng, n, k, q1), _text(rng, n, k, q2)
    taus = np.array([0, 1, 2, 3, 4, 5, 23], dtype=np.uint32)
    want1, want2 = ko.kmer_edist_both(c1, k, ko.singletons(q1, k), taus), ko.kmer_edist_both(c2, k, ko.singletons(q2, k), taus)
    assert not np.array_equal(want1[0], want2[0])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(_ascii(c1), 7)
        w = po.pack_codes(c1)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1, False)
        dt = _dev(taus, np.int32)
        e1, b1, d1 = _outputs(nq)
        e2, b2, d2 = _outputs(nq)
        n1, nb1, _ = _outputs(nq)
        n2, nb2, _ = _outputs(nq)

        def enqueue():
            c.kmer_edist_best_async(ptr, n, k, dq, nq, e1, d1)
            c.kmer_edist_count_multi_async(ptr, n, k, dq, dt, nq, n1)
            c.kmer_edist_best_packed_async(wptr, w.size, n, k, dq, nq, e2, d2)
            c.kmer_edist_count_multi_packed_async(wptr, w.size, n, k, dq, dt, nq, n2)

        def results():
            a, b = _read(c, e1, b1, nq), _read(c, e2, b2, nq)
            return {"ascii": (a[0], a[1], _read(c, n1, nb1, nq)[0]), "packed": (b[0], b[1], _read(c, n2, nb2, nq)[0])}

        enqueue()  # warm-up outside the capture: sizes the scratch
        _check(results(), want1, "warm-up")
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                enqueue()
            t[7:7 + n] = torch.from_numpy(_ascii(c2)).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(po.pack_codes(c2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2, False))
            for _ in range(2):
                for x in (e1, e2, n1, n2):
                    x.fill_(FILL)
                b1.fill_(0x5A)
                b2.fill_(0x5A)
                g.replay()
                _check(results(), want2, "replay")
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_with_hamming_calls_and_one_sync(ctx, oracle):
    """edit-distance and Hamming calls enqueued on one context (they share the context scratch of the keys and tables, in stream order), different query
    counts between consecutive calls, one sync at the end, every result checked afterwards"""
    import torch
    rng = np.random.default_rng(607)
    k, n = 21, 30_001
    dev = torch.device("cuda:0")
    jobs = []
    for i, nq in enumerate((5, 33, 1, 17, 4, 16, 2)):
        queries = _queries(rng, nq, k)
        codes = _text(rng, n + i, k, queries)
        taus = (np.arange(nq) % 5).astype(np.uint32)
        s = _ascii(codes, rng)
        w = po.pack_codes(codes)
        jobs.append(dict(i=i, nq=nq, queries=queries, codes=codes, s=s, taus=taus, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), w=w, wdev=_words_dev(w, i & 1),
                         dq=_dev_queries(queries, False), dt=_dev(taus, np.int32), out=_outputs(nq), cnt=_outputs(nq), hout=_outputs(nq),
                         hcnt=torch.zeros(nq, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, nq, m, ptr, dq = j["i"], j["nq"], j["s"].size, j["ascii"][1], j["dq"]
        if i % 2 == 0:
            ctx.kmer_edist_best_async(ptr, m, k, dq, nq, j["out"][0], j["out"][2])
            ctx.kmer_hdist_best_async(ptr, m, k, dq, nq, j["hout"][0], j["hout"][2])
            ctx.kmer_edist_count_multi_packed_async(j["wdev"][1], j["w"].size, m, k, dq, j["dt"], nq, j["cnt"][0])
        else:
            ctx.kmer_hdist_best_packed_async(j["wdev"][1], j["w"].size, m, k, dq, nq, j["hout"][0], j["hout"][2])
            ctx.kmer_edist_best_packed_async(j["wdev"][1], j["w"].size, m, k, dq, nq, j["out"][0], j["out"][2])
            ctx.kmer_edist_count_multi_async(ptr, m, k, dq, j["dt"], nq, j["cnt"][0])
        ctx.kmer_hdist_count_multi_dev(ptr, m, k, dq, j["dt"], nq, j["hcnt"])
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        nq, s, queries = j["nq"], j["s"], j["queries"]
        want = ko.kmer_edist_both(j["codes"], k, ko.singletons(queries, k), j["taus"])
        end, dist = _read(ctx, j["out"][0], j["out"][1], nq)
        cnt = _read(ctx, j["cnt"][0], j["cnt"][1], nq)[0]
        _check({"queue": (end, dist, cnt)}, want, j["i"])
        hp, hd = _read(ctx, j["hout"][0], j["hout"][1], nq)
        for q in range(nq):
            d = oracle.kmer_hdist_scan(s, k, int(queries[q]))
            assert (int(hp[q]), int(hd[q])) == (int(np.argmin(d)), int(np.min(d))) and int(j["hcnt"][q]) == int(np.count_nonzero(d <= int(j["taus"][q])))
        assert (dist <= hd).all() and (cnt >= j["hcnt"].cpu().numpy().view(np.uint64)).all()


# ---- 5. the host-pointer forms above the host cutoff ------------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context():
    import bitnuc_amd as bn
    rng = np.random.default_rng(809)
    n, k = 1_500_000, 23
    queries = _queries(rng, 3, k)
    codes = _text(rng, n, k, queries)
    s = _ascii(codes, rng)
    w = po.pack_codes(codes, junk=2**64 - 1)
    sing = ko.singletons(queries, k)
    taus = [0, 2, 5]
    want = ko.kmer_edist_both(codes, k, sing, taus)
    c = bn.Context(0)
    try:
        assert n * 3 >= 1 << 20
        for got in (c.kmer_edist_best(s, k, queries), c.kmer_edist_best_packed(w, n, k, queries), c.kmer_pattern_edist_best(s, k, sing),
                    c.kmer_pattern_edist_best_packed(w, n, k, sing)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for got in (c.kmer_edist_count_multi(s, k, queries, taus), c.kmer_edist_count_multi_packed(w, n, k, queries, taus),
                    c.kmer_pattern_edist_count_multi(s, k, sing, taus), c.kmer_pattern_edist_count_multi_packed(w, n, k, sing, taus)):
            assert np.array_equal(got, want[2])
        b = s.copy()
        b[n - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.kmer_edist_best(b, k, queries)
        assert (ei.value.byte, ei.value.index) == (ord("N"), n - 5)
        del ei
        assert np.array_equal(c.kmer_edist_count_multi(s, k, queries, taus), want[2])  # the next call is clean
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff run in chunks of 128 Mi end positions, each behind the 2k bases before it (packed: whole words), which are run
    but not reported.  An all-A reference of 128 Mi + 3 M bases with planted copies of a query without A (expected values: kmer_edist_oracle.sparse_both):
    a copy with one inserted base ACROSS the boundary (its last base 9 behind it: chunk 1 needs its lead-in), an exact copy that ends 30 bases before
    the boundary (inside chunk 1's lead-in: chunk 0 reports it, once), the same edited copy in both chunks (the leftmost end), and the count, in which a column of the overlap reported twice would show.  Then an
    N in chunk 1's lead-in and one past it report their absolute indices."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1282)
    chunk = 128 << 20
    n, k = chunk + 3_000_000, 25
    qs = [rng.integers(1, 4, size=k) for _ in range(3)]  # no A: the background is at distance k
    bulge = np.insert(qs[0], 12, 2)
    near = qs[2].copy()
    near[7] = near[7] % 3 + 1
    plants = [(chunk + 9 - len(bulge), bulge), (chunk - 30 - k, qs[1]), (5_000_000, near), (chunk + 1_000_000, near), (chunk + 2_000_000, qs[0][:k - 2])]
    queries = np.array([_word(q) for q in qs], dtype=np.uint64) | (np.uint64(0xABC) << np.uint64(2 * k))  # junk above 2k
    sing = ko.singletons(queries, k)
    taus = [1, 0, 1]
    want = [ko.sparse_both(n, plants, k, sing[q], taus[q]) for q in range(3)]
    assert [(int(e), int(d)) for e, d, _ in want] == [(chunk + 9, 1), (chunk - 30, 0), (5_000_000 + k, 1)] and [c for _, _, c in want] == [1, 1, 2]
    codes = np.zeros(n, dtype=np.uint8)
    for p, c in plants:
        codes[p:p + len(c)] = c
    s = LUT[codes]
    end, dist = ctx.kmer_edist_best(s, k, queries)
    assert [(int(e), int(d)) for e, d in zip(end, dist)] == [(int(e), int(d)) for e, d, _ in want]
    assert list(ctx.kmer_edist_count_multi(s, k, queries, taus)) == [c for _, _, c in want]
    w = oracle.encode(s)
    del codes
    end, dist = ctx.kmer_pattern_edist_best_packed(w, n, k, sing)
    assert [(int(e), int(d)) for e, d in zip(end, dist)] == [(int(e), int(d)) for e, d, _ in want]
    assert list(ctx.kmer_edist_count_multi_packed(w, n, k, queries, taus)) == [c for _, _, c in want]
    for at in (chunk - 3, chunk + 99):
        b = s[at]
        s[at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.kmer_edist_count_multi(s, k, queries, taus)
        assert (ei.value.byte, ei.value.index) == (ord("N"), at)
        del ei
        s[at] = b


# ---- 6. past 2^32 bases, across the grid's wrap ----------------------------------------------------------------------------------------------------
def test_packed_reference_past_32_bits(ctx):
    """2^32 + 70,000 bases of A as zero words, Q = 1: a copy of the query with two inserted bases just past base 2^32 and an exact copy near the end (the
    best), both at smaller distance than anywhere in the background; the expected values come from the oracle on the background's first 4k bases and on
    each plant's neighbourhood (kmer_edist_oracle.sparse_both).  A round of the bounded grid covers at most 2^29 bases, so this also crosses its wrap."""
    import torch
    dev = torch.device("cuda:0")
    n, k = (1 << 32) + 70_000, 31
    rng = np.random.default_rng(3232)
    qc = rng.integers(1, 4, size=k)
    bulge = np.insert(np.insert(qc, 20, 1), 9, 3)
    plants = [((1 << 32) + 40, bulge), (n - 1000, qc), (3 * (1 << 29) - 10, np.insert(qc, 15, 2))]  # the last: across the seam of two rounds of the grid
    p = ko.singletons([_word(qc)], k)[0]
    e_want, d_want, c_want = ko.sparse_both(n, plants, k, p, 2)
    assert (int(e_want), int(d_want)) == (n - 1000 + k, 0) and c_want >= 3
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    nw = (n + 31) // 32
    assert free >= 8 * nw + (1 << 28), f"needs {8 * nw / 2**30:.1f} GiB of device memory: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB"
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    for at, c in plants:  # the words that hold the plant, packed on the host
        w0, w1 = at // 32, (at + len(c) + 31) // 32
        local = np.zeros(32 * (w1 - w0), dtype=np.int64)
        local[at - 32 * w0:at - 32 * w0 + len(c)] = c
        words[w0:w1] = torch.from_numpy(po.pack_codes(local).view(np.int64)).to(dev)
    dq = _dev_queries([_word(qc)], False)
    dt = _dev(np.array([2], dtype=np.uint32), np.int32)
    e, db, dp = _outputs(1)
    c, cb, _ = _outputs(1)
    torch.cuda.synchronize()
    ctx.kmer_edist_best_packed_async(words, nw, n, k, dq, 1, e, dp)
    ctx.kmer_edist_count_multi_packed_async(words, nw, n, k, dq, dt, 1, c)
    end, dist = _read(ctx, e, db, 1)
    assert (int(end[0]), int(dist[0])) == (int(e_want), int(d_want))
    assert int(_read(ctx, c, cb, 1)[0][0]) == c_want
    # without the exact copy the bulge past 2^32 is the best: an end above 2^32 in the key and in end[]
    words[(n - 1000) // 32:(n - 1000 + k + 31) // 32] = 0
    e_want, d_want, _ = ko.sparse_both(n, [plants[0], plants[2]], k, p, 2)
    assert int(d_want) == 1 and int(e_want) == 3 * (1 << 29) - 10 + k + 1
    words[(3 * (1 << 29) - 10) // 32:(3 * (1 << 29) + k + 32) // 32] = 0
    e_want, d_want, _ = ko.sparse_both(n, [plants[0]], k, p, 2)
    assert int(d_want) == 2 and int(e_want) == (1 << 32) + 40 + k + 2
    e, db, dp = _outputs(1)
    torch.cuda.synchronize()
    ctx.kmer_edist_best_packed_async(words, nw, n, k, dq, 1, e, dp)
    end, dist = _read(ctx, e, db, 1)
    assert (int(end[0]), int(dist[0])) == (int(e_want), int(d_want))


# ---- 7. the C++ mirror ----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_of_the_kmer_edist_forms(ctx, tmp_path):
    """the eight kmer_*edist_* methods of include/bitnuc.hpp against the plain DP, via tests/cpp/test_kmer_edist_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kmer_edist_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_kmer_edist_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "kmer edist hpp ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
