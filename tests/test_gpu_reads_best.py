"""GPU tests of the best match per read (bitnuc_reads_hdist_best[_packed]_async, scan_reads_device.h): for every read of a fixed-length batch the
smallest (distance, query, offset) over all queries and the windows wholly inside the read, against tests/reads_best_oracle.py (numpy, or the oracle
library's contiguous scan masked and reduced per read) -- every k over read lengths below, at and across the segment / round / trip sizes with odd
periods, ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte and 8-mod-16 offsets with junk pad bits, query
counts around the query block; matches that straddle two reads (never seen); ties between registers, lanes, rounds, queries and query blocks; one
read walked by several trips of one wave; fills and limits; invalid bytes; a hipGraph replay; a queue of mixed asynchronous calls; the host forms
above the cutoff in one chunk and across two; a seeded differential fuzz.  Every comparison is exact equality of all three arrays; guard words and
bytes surround all three outputs and best_dist starts at an odd byte offset."""
import numpy as np
import pytest

import reads_best_oracle as ro

pytestmark = pytest.mark.gpu

QS = (1, 2, 15, 16, 17, 33, 257)
GUARD = 8
FILL32 = 0x5A5A5A5A
DOFF = 3
NO = ro.NO_U32


def _want(oracle, s, read_len, count, k, queries):
    """the numpy windows for small cases, the oracle's scan for large ones (both exact)"""
    if read_len >= k and count * (read_len - k + 1) * k * len(queries) > 2 * 10**7:
        return ro.reads_best_by_scan(oracle, s, read_len, count, k, queries)
    return ro.reads_best(s, read_len, count, k, queries)


def _dev_queries(queries):
    import torch
    return torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


class Out:
    """query / pos with GUARD words before and after [0, count); dist inside a guarded buffer, starting at the odd byte DOFF"""

    def __init__(self, count):
        import torch
        self.count = count
        self.q = torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
        self.p = torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
        self.d = torch.full((DOFF + count + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")

    def ptrs(self):
        return self.q.data_ptr() + 4 * GUARD, self.p.data_ptr() + 4 * GUARD, self.d.data_ptr() + DOFF

    def reset(self):
        self.q.fill_(FILL32)
        self.p.fill_(FILL32)
        self.d.fill_(0x5A)

    def untouched(self):
        return bool((self.q == FILL32).all()) and bool((self.p == FILL32).all()) and bool((self.d == 0x5A).all())

    def read(self, ctx=None):
        if ctx is not None:
            ctx.sync()
        n = self.count
        q, p, d = self.q.cpu().numpy().view(np.uint32), self.p.cpu().numpy().view(np.uint32), self.d.cpu().numpy()
        for a in (q, p):
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
        assert (d[:DOFF] == 0x5A).all() and (d[DOFF + n:] == 0x5A).all(), "dist written outside [0, count)"
        return q[GUARD:GUARD + n].copy(), p[GUARD:GUARD + n].copy(), d[DOFF:DOFF + n].copy()


def _ascii_dev(s, off):
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    return t, t.data_ptr() + off


def _words_dev(w, off):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off


def _both(ctx, s, read_len, count, k, queries, off=0, woff=0, words=None):
    """((query, pos, dist) of the ASCII form, ... of the packed form); guards checked"""
    import torch
    nq = len(queries)
    t, ptr = _ascii_dev(s, off)
    w = ro.pack_reads(s, read_len, count) if words is None else words
    tw, wptr = _words_dev(w, woff)
    dq = _dev_queries(queries)
    o1, o2 = Out(count), Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())
    ctx.reads_hdist_best_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
    got = o1.read(ctx), o2.read(ctx)
    del t, tw
    return got


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]) | (got[2] != want[2]))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


# ---- 1. every k, shape, query count and offset -------------------------------------------------------------------------------------
def _shapes(k):
    return ((k, 5000), (k + 1, 3000), (31, 2000), (33, 2000), (150, 300), (151, 2000), (1024, 9), (1056, 9), (4096, 5), (4097, 5), (70_001, 3))


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_shape_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(9100 + k)
    for si, (read_len, count) in enumerate(_shapes(k)):
        if read_len < k:
            continue
        nq = QS[(si + k) % len(QS)]
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        want = _want(oracle, s, read_len, count, k, queries)
        a, p = _both(ctx, s, read_len, count, k, queries, (0, 1, 7, 15)[(si + k) % 4], (si + k // 4) % 2)
        assert _same(a, want), ("ascii", k, read_len, count, nq, _diff(a, want))
        assert _same(p, want), ("packed", k, read_len, count, nq, _diff(p, want))


# ---- 2. windows that straddle two reads ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (20, 32))
@pytest.mark.parametrize("read_len", (40, 150, 1000))
def test_a_match_that_straddles_two_reads_is_not_seen(ctx, oracle, k, read_len):
    """Every split s in 1 .. k - 1: the first s bases of query 0 end read 2 s - 1, the other k - s start read 2 s.  The contiguous scan finds the
    copies at distance 0; no read may.  The packed form's pad bits above 2 * read_len hold the bases that would complete the match."""
    rng = np.random.default_rng(2200 + k + read_len)
    count = 2 * k + 1
    queries = ro.random_queries(rng, 3, k)
    qc = ro.query_codes(queries[0], k)
    codes = rng.integers(0, 4, size=(count, read_len))
    npad = 32 * ((read_len + 31) // 32) - read_len
    pad = rng.integers(0, 4, size=(count, npad))
    for s in range(1, k):
        r = 2 * s - 1
        codes[r, read_len - s:] = qc[:s]
        codes[r + 1, :k - s] = qc[s:]
        m = min(k - s, npad)
        pad[r, :m] = qc[s:s + m]  # what the next window positions of read r would need
    seq = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    seq[rng.random(seq.size) < 0.3] |= 0x20
    want = _want(oracle, seq, read_len, count, k, queries)
    assert (want[2] > 0).all() and (want[2] != 0xFF).all()
    scan = oracle.kmer_hdist_scan(seq, k, int(queries[0]))
    assert sorted(np.nonzero(scan == 0)[0]) == [(2 * s) * read_len - s for s in range(1, k)]
    words = ro.pack_reads(seq, read_len, count, pad_codes=pad)
    for off, woff in ((0, 0), (7, 1)):
        a, p = _both(ctx, seq, read_len, count, k, queries, off, woff, words=words)
        assert _same(a, want), ("ascii", _diff(a, want))
        assert _same(p, want), ("packed", _diff(p, want))


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup,nq", ((9, 24), (20, 24), (300, 304)))
def test_ties_the_lowest_query_then_the_lowest_offset(ctx, oracle, dup, nq):
    """The background holds no A and queries 3 and `dup` (the same query block, the next one, a far one) are k A's, every other query starts with A
    and is not all A: only the planted runs of k A's are at distance 0.  Reads 1 .. 4 hold two runs each, placed so that (ASCII, offset 0) they fall
    in two registers of one lane, two lanes of a round, two rounds of a trip and two trips; the lowest query and then the lowest offset must win."""
    rng = np.random.default_rng(3300 + dup)
    k, read_len, count = 8, 9000, 6
    codes = rng.integers(1, 4, size=(count, read_len))
    pairs = {1: (216, 224), 2: (3000, 3100), 3: (500, 500 + 1024), 4: (100, 100 + 4096 + 50)}  # run position 9000 + 216 = 9216 = 9 * 1024: register 0 and 4 of lane 0
    for r, (i1, i2) in pairs.items():
        codes[r, i1:i1 + k] = 0
        codes[r, i2:i2 + k] = 0
    queries = ro.random_queries(rng, nq, k)
    queries &= ~np.uint64(3)  # position 0: A
    queries |= np.uint64(1) << np.uint64(2 * 5)  # position 5: not A
    for q in (3, dup):
        queries[q] &= ~np.uint64((1 << (2 * k)) - 1)  # k A's, junk above 2k kept
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = _want(oracle, s, read_len, count, k, queries)
    for r, (i1, _) in pairs.items():
        assert (int(want[0][r]), int(want[1][r]), int(want[2][r])) == (3, i1, 0)
    assert want[2][0] > 0 and want[2][5] > 0
    for off, woff in ((0, 0), (15, 1)):
        a, p = _both(ctx, s, read_len, count, k, queries, off, woff)
        assert _same(a, want), ("ascii", _diff(a, want))
        assert _same(p, want), ("packed", _diff(p, want))


# ---- 4. one long read walked by several trips of one wave -------------------------------------------------------------------------------
def test_one_read_walked_by_several_trips_of_one_wave(ctx, oracle):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    read_len = cus * 12 * 4 * 1024 + 10**6 + 13  # more rounds than the grid's waves x a trip: some wave walks a second trip inside read 0
    count, k = 2, 27
    rng = np.random.default_rng(44)
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=count * read_len).astype(np.uint8)
    q0, q1 = ro.query_codes(queries[0], k), ro.query_codes(queries[1], k)
    near = q0.copy()
    near[3] ^= 1
    codes[1000:1000 + k] = near                            # read 0: query 0 with one change in the first trip ...
    codes[read_len - 500_000:read_len - 500_000 + k] = q0  # ... and exactly in a later trip of the walk: the closer one wins
    codes[read_len + 70_000:read_len + 70_000 + k] = q1    # read 1: query 1 twice
    codes[2 * read_len - k:2 * read_len] = q1              # ... the second time at its last window
    s = ro.LUT[codes]
    del codes
    want = ro.reads_best_by_scan(oracle, s, read_len, count, k, queries)
    assert [tuple(int(a[r]) for a in want) for r in (0, 1)] == [(0, read_len - 500_000, 0), (1, 70_000, 0)]
    a, p = _both(ctx, s, read_len, count, k, queries, 1, 1)
    assert _same(a, want), ("ascii", _diff(a, want))
    assert _same(p, want), ("packed", _diff(p, want))


# ---- 5. fills and limits -----------------------------------------------------------------------------------------------------------------
def test_no_window_fills_and_count_zero(ctx):
    import torch
    s = ro.LUT[np.random.default_rng(1).integers(0, 4, size=3000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(ro.pack_reads(s, 30, 100), 1)
    dq = _dev_queries([1, 2, 3])
    for read_len, k, nq in ((5, 6, 3), (30, 0, 3), (30, 5, 0)):
        for fn, src in ((ctx.reads_hdist_best_async, ptr), (ctx.reads_hdist_best_packed_async, wptr)):
            o = Out(100)
            torch.cuda.synchronize()
            fn(src, read_len, 100, k, dq if nq else None, nq, *o.ptrs())
            q, p, d = o.read(ctx)
            assert (q == NO).all() and (p == NO).all() and (d == 0xFF).all(), (read_len, k, nq)
    for fn, src in ((ctx.reads_hdist_best_async, ptr), (ctx.reads_hdist_best_packed_async, wptr)):
        o = Out(4)
        torch.cuda.synchronize()
        fn(src, 30, 0, 5, dq, 3, *o.ptrs())  # count == 0: nothing written
        ctx.sync()
        assert o.untouched()


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries in one call (4096 query blocks) on a small batch, against the host form in slices merged in (dist, query) order."""
    from bitnuc_amd import api
    rng = np.random.default_rng(65536)
    k, read_len, count, nq = 12, 60, 40, 65536
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries[60000:], plant=8)
    free = api.context_free()
    assert _same(free.reads_hdist_best(s, read_len, k, queries[:64]), ro.reads_best(s, read_len, count, k, queries[:64]))
    full = ro.fill(count)
    for i in range(0, nq, 256):
        q, p, d = free.reads_hdist_best(s, read_len, k, queries[i:i + 256])
        take = d < full[2]  # slices in ascending order: a later one wins on a strictly smaller distance only
        full[0][take], full[1][take], full[2][take] = q[take] + np.uint32(i), p[take], d[take]
    a, p = _both(ctx, s, read_len, count, k, queries, 1, 1)
    assert _same(a, full), _diff(a, full)
    assert _same(p, full), _diff(p, full)


def test_argument_errors_leave_the_outputs_untouched(ctx):
    import torch
    import bitnuc_amd as bn
    s = ro.LUT[np.random.default_rng(2).integers(0, 4, size=6000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(ro.pack_reads(s, 60, 100), 0)
    dq = _dev_queries(np.zeros(16, dtype=np.uint64))
    o = Out(100)
    bq, bp, bd = o.ptrs()
    torch.cuda.synchronize()
    for fn, src in ((ctx.reads_hdist_best_async, ptr), (ctx.reads_hdist_best_packed_async, wptr)):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 12, dq, 65537, bq, bp, bd)
        assert ei.value.kind == "Unsupported"
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 33, dq, 16, bq, bp, bd)
        assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 12, dq, 16, bq, bp + 2, bd)  # best_pos not 4-byte aligned
        assert ei.value.kind == "Unsupported"
        del ei
    ctx.sync()
    assert o.untouched()


# ---- 6. invalid bytes ----------------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_reported_once_with_the_first_index(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(6)
    k, read_len, count, nq = 17, 150, 400, 33
    n = read_len * count
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    want = _want(oracle, s, read_len, count, k, queries)
    dq = _dev_queries(queries)
    for bad_at, off in ((31_337, 0), (n - 3, 5), (2, 9), (n - 20, 0)):  # a middle round, the last read's tail (twice: its last k - 1 bases), the head
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *o.ptrs())
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing left for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best_async(ptr2, read_len, count, k, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), want)


# ---- 7. hipGraph ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reads_and_the_queries_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(77)
    read_len, count, k, nq = 151, 2000, 31, 33
    q1, q2 = ro.random_queries(rng, nq, k), ro.random_queries(rng, nq, k)
    s1, s2 = ro.random_reads(rng, read_len, count, k, q1), ro.random_reads(rng, read_len, count, k, q2)
    want1, want2 = _want(oracle, s1, read_len, count, k, q1), _want(oracle, s2, read_len, count, k, q2)
    assert not np.array_equal(want1[1], want2[1])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = ro.pack_reads(s1, read_len, count)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        o1, o2 = Out(count), Out(count)
        c.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())  # warm-up outside the capture: sizes the scratch
        c.reads_hdist_best_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())
                c.reads_hdist_best_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(ro.pack_reads(s2, read_len, count).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2))
            for _ in range(2):
                o1.reset()
                o2.reset()
                g.replay()
                assert _same(o1.read(c), want2) and _same(o2.read(c), want2)
        finally:
            g.reset()
            del g
            c.close()


# ---- 8. a queue of mixed asynchronous calls ----------------------------------------------------------------------------------------------
def test_mixed_queue_with_one_sync(ctx, oracle):
    """reads_best and reads_best_packed between kmer_hdist_best, count_multi, encode_fixed and hits on one context, different (count, n_queries)
    between consecutive calls (the scratch slot's keys and tables are rewritten by each), one sync at the end, every result checked afterwards."""
    import torch
    rng = np.random.default_rng(808)
    k, read_len = 21, 150
    dev = torch.device("cuda:0")
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2))):  # inputs and outputs first
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        taus = (np.arange(nq) % 5).astype(np.uint32)
        wpr = (read_len + 31) // 32
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, taus=taus, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         out=Out(count), wdev=_words_dev(ro.pack_reads(s, read_len, count), i & 1),
                         dt=torch.from_numpy(taus.view(np.int32)).to(dev), counts=torch.zeros(nq, dtype=torch.int64, device=dev),
                         hp=torch.zeros(64, dtype=torch.int64, device=dev), nh=torch.zeros(1, dtype=torch.int64, device=dev),
                         bpos=torch.zeros(nq, dtype=torch.int64, device=dev), bdist=torch.zeros(nq, dtype=torch.uint8, device=dev),
                         words=torch.zeros(count * wpr, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    calls = 0
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, s, ptr, dq = j["i"], j["count"], j["nq"], j["s"], j["ascii"][1], j["dq"]
        if i % 2 == 0:
            ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *j["out"].ptrs())
        else:
            ctx.reads_hdist_best_packed_async(j["wdev"][1], read_len, count, k, dq, nq, *j["out"].ptrs())
        if i % 4 == 0:
            ctx.kmer_hdist_count_multi_dev(ptr, s.size, k, dq, j["dt"], nq, j["counts"])
        elif i % 4 == 1:
            ctx.kmer_hdist_hits_dev(ptr, s.size, k, int(j["queries"][0]), 3, j["hp"], None, 64, j["nh"])
        elif i % 4 == 2:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, j["bpos"], j["bdist"])
        else:
            ctx.encode_fixed_dev(ptr, read_len, read_len, count, j["words"])
        calls += 2
    assert calls >= 12
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, count, nq, s, queries = j["i"], j["count"], j["nq"], j["s"], j["queries"]
        want = _want(oracle, s, read_len, count, k, queries)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        scans = [oracle.kmer_hdist_scan(s, k, int(q)) for q in queries]
        if i % 4 == 0:
            assert j["counts"].cpu().tolist() == [int(np.count_nonzero(d <= int(t))) for d, t in zip(scans, j["taus"])], i
        elif i % 4 == 1:
            wh = np.nonzero(scans[0] <= 3)[0]
            assert int(j["nh"][0]) == wh.size and j["hp"].cpu().tolist()[:min(64, wh.size)] == list(wh[:64]), i
        elif i % 4 == 2:
            assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i
        else:
            assert np.array_equal(j["words"].cpu().numpy().view(np.uint64), ro.pack_reads(s, read_len, count, junk=False)), i


# ---- 9. the host-pointer forms above the host cutoff ---------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context(oracle):
    """20,000 reads of 150 bases and three queries (8 * 10^6 window-query pairs, above the default cutoff of 2^20) on a context with the default
    dispatch run through the device in one chunk; the same calls below the cutoff and one query passed as a number give the same answers."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(909)
    read_len, count, k = 150, 20_000, 23
    queries = ro.random_queries(rng, 3, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    want = ro.reads_best_by_scan(oracle, s, read_len, count, k, queries)
    words = ro.pack_reads(s, read_len, count)
    c = bn.Context(0)
    try:
        assert count * (read_len - k + 1) * 3 >= 1 << 20
        assert _same(c.reads_hdist_best(s, read_len, k, queries), want)
        assert _same(c.reads_hdist_best_packed(words, read_len, count, k, queries), want)
        one = c.reads_hdist_best(s, read_len, k, int(queries[1]))  # a scalar query: Q = 1
        assert _same(one, ro.reads_best_by_scan(oracle, s, read_len, count, k, queries[1:2]))
        m = 1000  # 3.8 * 10^5 pairs: the same call stays on the host
        assert _same(c.reads_hdist_best(s[:m * read_len], read_len, k, queries), tuple(a[:m] for a in want))
        b = s.copy()
        b[s.size - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_hdist_best(b, read_len, k, queries)
        assert (ei.value.byte, ei.value.index) == (ord("N"), s.size - 5)
        del ei
        assert _same(c.reads_hdist_best(s, read_len, k, queries), want)  # the next call is clean
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """900,000 reads of 150 bases: the ASCII form's chunks are 894,784 whole reads (128 Mi bytes / 150), the packed form's 838,860 (4 Mi words / 5);
    no read is split, so the reads on both sides of each boundary -- which hold planted copies at their first and last windows -- get their own
    answers.  Then an N past the boundary reports its absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1282)
    read_len, count, k = 150, 900_000, 25
    per_ascii, per_packed = (128 << 20) // read_len, ((128 << 20) // 32) // 5
    assert per_packed < per_ascii < count
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    for per in (per_ascii, per_packed):
        codes[per - 1, read_len - k:] = qc[0]  # the last window of the chunk's last read
        codes[per, :k] = qc[1]                 # the first window of the next chunk's first read
        codes[per + 1, 60:60 + k] = qc[0]
    s = ro.LUT[codes.reshape(-1)]
    del codes
    want = ro.reads_best_by_scan(oracle, s, read_len, count, k, queries)
    for per in (per_ascii, per_packed):
        assert [tuple(int(a[r]) for a in want) for r in (per - 1, per, per + 1)] == [(0, read_len - k, 0), (1, 0, 0), (0, 60, 0)]
    got = ctx.reads_hdist_best(s, read_len, k, queries)
    assert _same(got, want), _diff(got, want)
    words = ctx.encode_fixed(s, read_len).reshape(-1)  # (the library's own fixed-length encoder: zero pad bits)
    assert np.array_equal(words[:50], ro.pack_reads(s, read_len, 10, junk=False))
    got = ctx.reads_hdist_best_packed(words, read_len, count, k, queries)
    assert _same(got, want), _diff(got, want)
    bad_at = per_ascii * read_len + 99
    s[bad_at] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.reads_hdist_best(s, read_len, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
    del ei


# ---- 10. seeded differential fuzz ------------------------------------------------------------------------------------------------------------
def test_seeded_differential_fuzz(ctx, oracle):
    rng = np.random.default_rng(0xF022)
    for it in range(200):
        k = int(rng.integers(1, 33))
        read_len = int(rng.integers(k, 401))
        count = int(rng.integers(1, (3001, 300, 40, 300)[it % 4]))  # up to 3000 reads, most cases smaller
        nq = int(rng.integers(1, 41))
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        want = ro.reads_best_by_scan(oracle, s, read_len, count, k, queries)
        a, p = _both(ctx, s, read_len, count, k, queries, int(rng.integers(0, 16)), int(rng.integers(0, 2)))
        assert _same(a, want), ("ascii", it, k, read_len, count, nq, _diff(a, want))
        assert _same(p, want), ("packed", it, k, read_len, count, nq, _diff(p, want))
