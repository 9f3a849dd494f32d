"""GPU tests of the best match and the runner-up per read (bitnuc_reads_hdist_best2[_packed]_async and the host forms above the cutoff;
scan_reads_device.h's exclusion form) against tests/reads_best2_oracle.py: every k over read lengths below, at and across the segment / round / trip
sizes with odd periods and query counts around the query block; the exclusion per read where a lane's segment spans two reads with different
winners; the winner's own second window; ties between equal queries; matches that straddle two reads; one read walked by several trips of one wave;
fills, the query limit and argument errors; invalid bytes; a hipGraph replay; a queue of mixed asynchronous calls; the host forms in one chunk and
across two; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte and 8-mod-16
offsets with junk pad bits run on the same data.  Every comparison is exact equality of all six arrays; guard words and bytes surround all six
outputs and both dist arrays start at odd byte offsets; wherever both device forms run, the first three outputs are also held against
reads_hdist_best*_async's on the same inputs."""
import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2

pytestmark = pytest.mark.gpu

QS = (1, 2, 15, 16, 17, 33, 257)
GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
NO = ro.NO_U32


def _want(oracle, s, read_len, count, k, queries):
    """the numpy windows for small cases, the oracle's scan for large ones (both exact)"""
    if read_len >= k and count * (read_len - k + 1) * k * len(queries) > 2 * 10**7:
        return r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)
    return r2.reads_best2(s, read_len, count, k, queries)


def _dev_queries(queries):
    import torch
    return torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


class Out:
    """`triples` x (query / pos with GUARD words before and after [0, count); dist inside a guarded buffer, starting at an odd byte)"""

    def __init__(self, count, triples=2):
        import torch
        self.count = count
        self.w = [torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(2 * triples)]
        self.d = [torch.full((off + count + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0") for off in DOFFS[:triples]]

    def ptrs(self):
        out = []
        for j, d in enumerate(self.d):
            out += [self.w[2 * j].data_ptr() + 4 * GUARD, self.w[2 * j + 1].data_ptr() + 4 * GUARD, d.data_ptr() + DOFFS[j]]
        return out

    def reset(self):
        for a in self.w:
            a.fill_(FILL32)
        for a in self.d:
            a.fill_(0x5A)

    def untouched(self):
        return all(bool((a == FILL32).all()) for a in self.w) and all(bool((a == 0x5A).all()) for a in self.d)

    def read(self, ctx=None):
        if ctx is not None:
            ctx.sync()
        n = self.count
        out = []
        for j, d in enumerate(self.d):
            for a in self.w[2 * j:2 * j + 2]:
                a = a.cpu().numpy().view(np.uint32)
                assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
                out.append(a[GUARD:GUARD + n].copy())
            d = d.cpu().numpy()
            assert (d[:DOFFS[j]] == 0x5A).all() and (d[DOFFS[j] + n:] == 0x5A).all(), "dist written outside [0, count)"
            out.append(d[DOFFS[j]:DOFFS[j] + n].copy())
        return tuple(out)


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


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero(np.any([g != w for g, w in zip(got, want)], axis=0))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


def _both(ctx, s, read_len, count, k, queries, off=0, woff=0, words=None):
    """(six arrays of the ASCII form, six of the packed form); guards checked, and the best triples held against reads_hdist_best*_async's"""
    import torch
    nq = len(queries)
    t, ptr = _ascii_dev(s, off)
    w = ro.pack_reads(s, read_len, count) if words is None else words
    tw, wptr = _words_dev(w, woff)
    dq = _dev_queries(queries)
    o1, o2, b1, b2 = Out(count), Out(count), Out(count, 1), Out(count, 1)
    torch.cuda.synchronize()
    ctx.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())
    ctx.reads_hdist_best2_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
    ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *b1.ptrs())
    ctx.reads_hdist_best_packed_async(wptr, read_len, count, k, dq, nq, *b2.ptrs())
    ctx.sync()
    got = o1.read(), o2.read()
    assert _same(got[0][:3], b1.read()), ("ascii: the best triple is not reads_hdist_best_async's", _diff(got[0][:3], b1.read()))
    assert _same(got[1][:3], b2.read()), ("packed: the best triple is not reads_hdist_best_packed_async's", _diff(got[1][:3], b2.read()))
    del t, tw
    return got


def _check(ctx, s, read_len, count, k, queries, want, off=0, woff=0, words=None, tag=()):
    a, p = _both(ctx, s, read_len, count, k, queries, off, woff, words)
    assert _same(a, want), ("ascii", tag, _diff(a, want))
    assert _same(p, want), ("packed", tag, _diff(p, want))


def _row(want, r):
    return tuple(int(a[r]) for a in want)


# ---- 1. every k, shape, query count and offset -------------------------------------------------------------------------------------
def _shapes(k):
    return ((k, 600), (k + 1, 400), (33, 400), (150, 200), (151, 300), (1056, 9), (4097, 5), (70_001, 3))


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_shape_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(9200 + k)
    for si, (read_len, count) in enumerate(_shapes(k)):
        nq = QS[(si + k) % len(QS)]
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        want = _want(oracle, s, read_len, count, k, queries)
        _check(ctx, s, read_len, count, k, queries, want, (0, 1, 7, 15)[(si + k) % 4], (si + k // 4) % 2, tag=(k, read_len, count, nq))


# ---- 2. the exclusion is per read, not per lane ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", (40, 150))
def test_exclusion_is_per_read_where_a_segment_spans_two_reads(ctx, oracle, read_len):
    """Reads 2 j and 2 j + 1 have different winners, queries 2 and 5.  The even read ends in a distance-1 copy of query 5 (its last window), the odd one
    starts with a distance-1 copy of query 2 (its first window): the segment of 32 windows across their boundary must leave out 2 for the read before
    the boundary and 5 for the one after it."""
    rng = np.random.default_rng(1200 + read_len)
    k, count, nq = 12, 64, 8
    queries = ro.random_queries(rng, nq, k)
    q2, q5 = ro.query_codes(queries[2], k), ro.query_codes(queries[5], k)
    n2, n5 = q2.copy(), q5.copy()
    n2[4] ^= 1
    n5[9] ^= 2
    codes = rng.integers(0, 4, size=(count, read_len))
    at2, at5 = (0, 18) if read_len == 40 else (30, 70)
    for r in range(0, count, 2):
        codes[r, at2:at2 + k] = q2
        codes[r, read_len - k:] = n5
        codes[r + 1, :k] = n2
        codes[r + 1, at5:at5 + k] = q5
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    s[rng.random(s.size) < 0.3] |= 0x20
    want = _want(oracle, s, read_len, count, k, queries)
    for r in range(0, count, 2):
        assert _row(want, r) == (2, at2, 0, 5, read_len - k, 1) and _row(want, r + 1) == (5, at5, 0, 2, 0, 1)
    for off, woff in ((0, 0), (7, 1), (15, 0)):
        _check(ctx, s, read_len, count, k, queries, want, off, woff)


# ---- 3. the winner's own second window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,run,nq", ((3, 7, 24), (3, 20, 24), (3, 300, 304), (20, 7, 24)))
def test_the_winners_second_window_is_never_the_runner_up(ctx, oracle, win, run, nq):
    """Query `win` at distances 0 and 1 in one read, query `run` at distance 2 (the same query block, the next one, a far one; and a LOWER query at a
    greater distance): the runner-up is `run`, not the winner's second window."""
    rng = np.random.default_rng(3400 + win + run)
    k, read_len, count = 16, 150, 40
    queries = ro.random_queries(rng, nq, k)
    qw, qr = ro.query_codes(queries[win], k), ro.query_codes(queries[run], k)
    w1, r2c = qw.copy(), qr.copy()
    w1[5] ^= 3
    r2c[2] ^= 1
    r2c[13] ^= 2
    codes = rng.integers(0, 4, size=(count, read_len))
    places = {}
    for r in range(1, count, 3):  # the three copies in every order, at offsets that move through the segments
        p = [2 + (r % 5), 50 + (r % 7), 110 + (r % 11)]
        order = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)][(r // 3) % 6]
        places[r] = (p[order[0]], p[order[2]])
        codes[r, p[order[0]]:p[order[0]] + k] = qw
        codes[r, p[order[1]]:p[order[1]] + k] = w1
        codes[r, p[order[2]]:p[order[2]] + k] = r2c
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = _want(oracle, s, read_len, count, k, queries)
    for r, (pw, pr) in places.items():
        assert _row(want, r) == (win, pw, 0, run, pr, 2), (r, _row(want, r))
    for off, woff in ((0, 0), (1, 1)):
        _check(ctx, s, read_len, count, k, queries, want, off, woff)


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup,nq", ((9, 24), (20, 24), (300, 304)))
def test_ties_an_equal_query_is_the_runner_up_at_the_first_run(ctx, oracle, dup, nq):
    """The background holds no A and queries 3 and `dup` (the same query block, the next one, a far one) are k A's, every other query starts and ends with
    an A and has another base in between -- a window with A's at both ends lies inside a run of A's --: only the two are at distance 0 anywhere.  Reads 1 .. 4 hold two runs each, placed so that (ASCII, offset 0) they fall
    in two registers of one lane, two lanes of a round, two rounds of a trip and two trips: best = (0, 3, first run), runner-up = (0, dup, first
    run)."""
    rng = np.random.default_rng(3300 + dup)
    k, read_len, count = 8, 9000, 6
    codes = rng.integers(1, 4, size=(count, read_len))
    pairs = {1: (216, 224), 2: (3000, 3100), 3: (500, 500 + 1024), 4: (100, 100 + 4096 + 50)}  # run position 9000 + 216 = 9216 = 9 * 1024: register 0 and 4 of lane 0
    for r, (i1, i2) in pairs.items():
        codes[r, i1:i1 + k] = 0
        codes[r, i2:i2 + k] = 0
    queries = ro.random_queries(rng, nq, k)
    queries &= ~np.uint64(3 | (3 << (2 * (k - 1))))  # positions 0 and k - 1: A
    queries |= np.uint64(1) << np.uint64(2 * 5)  # position 5: not A
    for q in (3, dup):
        queries[q] &= ~np.uint64((1 << (2 * k)) - 1)  # k A's, junk above 2k kept
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = _want(oracle, s, read_len, count, k, queries)
    for r, (i1, _) in pairs.items():
        assert _row(want, r) == (3, i1, 0, dup, i1, 0)
    assert want[2][0] > 0 and want[2][5] > 0
    for off, woff in ((0, 0), (15, 1)):
        _check(ctx, s, read_len, count, k, queries, want, off, woff)


# ---- 5. windows that straddle two reads ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", (40, 150))
def test_a_match_that_straddles_two_reads_is_seen_by_neither_triple(ctx, oracle, read_len):
    """Every split s in 1 .. k - 1: the first s bases of query 0 end read 2 s - 1, the other k - s start read 2 s.  The contiguous scan finds the
    copies at distance 0; no read may, as best or as runner-up.  The packed form's pad bits above 2 * read_len hold the bases that would complete the
    match."""
    k = 20
    rng = np.random.default_rng(2300 + read_len)
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
    assert (want[2] > 0).all() and (want[2] != 0xFF).all() and (want[5] > 0).all() and (want[5] != 0xFF).all()
    scan = oracle.kmer_hdist_scan(seq, k, int(queries[0]))
    assert sorted(np.nonzero(scan == 0)[0]) == [(2 * s) * read_len - s for s in range(1, k)]
    words = ro.pack_reads(seq, read_len, count, pad_codes=pad)
    for off, woff in ((0, 0), (7, 1)):
        _check(ctx, seq, read_len, count, k, queries, want, off, woff, words=words)


# ---- 6. one long read walked by several trips of one wave -------------------------------------------------------------------------------
def test_one_read_walked_by_several_trips_of_one_wave(ctx, oracle):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    read_len = cus * 12 * 4 * 1024 + 10**6 + 13  # more rounds than the grid's waves x a trip: some wave walks a second trip inside read 0
    count, k = 2, 27
    rng = np.random.default_rng(45)
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=count * read_len).astype(np.uint8)
    q0, q1 = ro.query_codes(queries[0], k), ro.query_codes(queries[1], k)
    near = q1.copy()
    near[3] ^= 1
    codes[1000:1000 + k] = near                            # read 0: query 1 with one change in the first trip: the runner-up ...
    codes[read_len - 500_000:read_len - 500_000 + k] = q0  # ... and query 0 exactly in a later trip of the walk: the winner
    codes[read_len + 70_000:read_len + 70_000 + k] = q1    # read 1: query 1 twice
    codes[2 * read_len - k:2 * read_len] = q1              # ... the second time at its last window
    s = ro.LUT[codes]
    del codes
    want = r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)
    assert _row(want, 0) == (0, read_len - 500_000, 0, 1, 1000, 1) and _row(want, 1)[:4] == (1, 70_000, 0, 0)
    _check(ctx, s, read_len, count, k, queries, want, 1, 1)


# ---- 7. fills, limits and argument errors ----------------------------------------------------------------------------------------------------
def test_fills_no_window_one_query_and_count_zero(ctx):
    import torch
    rng = np.random.default_rng(1)
    s = ro.LUT[rng.integers(0, 4, size=3000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(ro.pack_reads(s, 30, 100), 1)
    queries = ro.random_queries(rng, 3, 5)
    dq = _dev_queries(queries)
    forms = ((ctx.reads_hdist_best2_async, ptr), (ctx.reads_hdist_best2_packed_async, wptr))
    for read_len, k, nq in ((5, 6, 3), (30, 0, 3), (30, 5, 0)):  # no window: all six
        for fn, src in forms:
            o = Out(100)
            torch.cuda.synchronize()
            fn(src, read_len, 100, k, dq if nq else None, nq, *o.ptrs())
            assert _same(o.read(ctx), r2.fill6(100)), (read_len, k, nq)
    want = r2.reads_best2(s, 30, 100, 5, queries[:1])  # one query: the best triple is real, the second the fill
    assert (want[2] != 0xFF).all() and (want[3] == NO).all() and (want[4] == NO).all() and (want[5] == 0xFF).all()
    for fn, src in forms:
        o = Out(100)
        torch.cuda.synchronize()
        fn(src, 30, 100, 5, dq, 1, *o.ptrs())
        assert _same(o.read(ctx), want)
    for fn, src in forms:
        o = Out(4)
        torch.cuda.synchronize()
        fn(src, 30, 0, 5, dq, 3, *o.ptrs())  # count == 0: nothing written
        ctx.sync()
        assert o.untouched()


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries in one call (4096 query blocks) on a small batch, against the host form in slices of 256 merged by a top-2 merge over
    distinct queries (reads_best2_oracle.merge_top2)."""
    from bitnuc_amd import api
    rng = np.random.default_rng(65537)
    k, read_len, count, nq = 12, 60, 40, 65536
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries[60000:], plant=8)
    free = api.context_free()
    assert _same(free.reads_hdist_best2(s, read_len, k, queries[:64]), r2.reads_best2(s, read_len, count, k, queries[:64]))
    full = r2.merge_top2([(i, free.reads_hdist_best2(s, read_len, k, queries[i:i + 256])) for i in range(0, nq, 256)])
    assert (full[5] != 0xFF).all()
    _check(ctx, s, read_len, count, k, queries, full, 1, 1)


def test_argument_errors_leave_the_outputs_untouched(ctx):
    import torch
    import bitnuc_amd as bn
    s = ro.LUT[np.random.default_rng(2).integers(0, 4, size=6000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(ro.pack_reads(s, 60, 100), 0)
    dq = _dev_queries(np.zeros(16, dtype=np.uint64))
    o = Out(100)
    six = o.ptrs()
    torch.cuda.synchronize()
    for fn, src in ((ctx.reads_hdist_best2_async, ptr), (ctx.reads_hdist_best2_packed_async, wptr)):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 12, dq, 65537, *six)
        assert ei.value.kind == "Unsupported"
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 33, dq, 16, *six)
        assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 60, 100, 12, dq, 16, six[0], six[1], six[2], six[3] + 2, six[4], six[5])  # second_query not 4-byte aligned
        assert ei.value.kind == "Unsupported"
        del ei
    ctx.sync()
    assert o.untouched()


# ---- 8. invalid bytes ----------------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_reported_once_with_the_first_index(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, read_len, count, nq = 17, 150, 400, 33
    n = read_len * count
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    want = _want(oracle, s, read_len, count, k, queries)
    dq = _dev_queries(queries)
    for bad_at, off in ((31_337, 0), (2, 9), (n - 3, 5)):  # a middle round, the head, the last read's last k - 1 bases
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *o.ptrs())
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: the second pass has left nothing for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean and correct
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best2_async(ptr2, read_len, count, k, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), want)


# ---- 9. hipGraph ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reads_and_the_queries_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    read_len, count, k, nq = 151, 2000, 31, 33
    q1, q2 = ro.random_queries(rng, nq, k), ro.random_queries(rng, nq, k)
    s1, s2 = ro.random_reads(rng, read_len, count, k, q1), ro.random_reads(rng, read_len, count, k, q2)
    want1, want2 = _want(oracle, s1, read_len, count, k, q1), _want(oracle, s2, read_len, count, k, q2)
    assert not np.array_equal(want1[1], want2[1]) and not np.array_equal(want1[4], want2[4])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = ro.pack_reads(s1, read_len, count)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        o1, o2 = Out(count), Out(count)
        c.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())  # warm-up outside the capture: sizes the scratch
        c.reads_hdist_best2_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())
                c.reads_hdist_best2_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
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


# ---- 10. a queue of mixed asynchronous calls ----------------------------------------------------------------------------------------------
def test_mixed_queue_with_one_sync(ctx, oracle):
    """best2 (ASCII and packed in turn) between reads_hdist_best, kmer_hdist_best, count_multi and encode_fixed on one context, different (count,
    n_queries) between consecutive calls (the scratch slot's key arrays and tables are laid out anew by each), one sync at the end, every result
    checked afterwards."""
    import torch
    rng = np.random.default_rng(809)
    k, read_len = 21, 150
    dev = torch.device("cuda:0")
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (800, 3))):  # inputs and outputs first
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        taus = (np.arange(nq) % 5).astype(np.uint32)
        wpr = (read_len + 31) // 32
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, taus=taus, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         out=Out(count), one=Out(count, 1), wdev=_words_dev(ro.pack_reads(s, read_len, count), i & 1),
                         dt=torch.from_numpy(taus.view(np.int32)).to(dev), counts=torch.zeros(nq, dtype=torch.int64, device=dev),
                         bpos=torch.zeros(nq, dtype=torch.int64, device=dev), bdist=torch.zeros(nq, dtype=torch.uint8, device=dev),
                         words=torch.zeros(count * wpr, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, s, ptr, dq = j["i"], j["count"], j["nq"], j["s"], j["ascii"][1], j["dq"]
        if i % 2 == 0:
            ctx.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *j["out"].ptrs())
        else:
            ctx.reads_hdist_best2_packed_async(j["wdev"][1], read_len, count, k, dq, nq, *j["out"].ptrs())
        if i % 4 == 0:
            ctx.kmer_hdist_count_multi_dev(ptr, s.size, k, dq, j["dt"], nq, j["counts"])
        elif i % 4 == 1:
            ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *j["one"].ptrs())
        elif i % 4 == 2:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, j["bpos"], j["bdist"])
        else:
            ctx.encode_fixed_dev(ptr, read_len, read_len, count, j["words"])
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, count, nq, s, queries = j["i"], j["count"], j["nq"], j["s"], j["queries"]
        want = _want(oracle, s, read_len, count, k, queries)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        if i % 4 == 1:
            assert _same(j["one"].read(), want[:3]), i
        elif i % 4 == 3:
            assert np.array_equal(j["words"].cpu().numpy().view(np.uint64), ro.pack_reads(s, read_len, count, junk=False)), i
        else:
            scans = [oracle.kmer_hdist_scan(s, k, int(q)) for q in queries]
            if i % 4 == 0:
                assert j["counts"].cpu().tolist() == [int(np.count_nonzero(d <= int(t))) for d, t in zip(scans, j["taus"])], i
            else:
                assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i


# ---- 11. the host-pointer forms above the host cutoff ---------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context(oracle):
    """20,000 reads of 150 bases and three queries (8 * 10^6 window-query pairs, above the default cutoff of 2^20) on a context with the default
    dispatch run through the device in one chunk; the same call below the cutoff and one query passed as a number give the same answers."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(910)
    read_len, count, k = 150, 20_000, 23
    queries = ro.random_queries(rng, 3, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    want = r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)
    words = ro.pack_reads(s, read_len, count)
    c = bn.Context(0)
    try:
        assert count * (read_len - k + 1) * 3 >= 1 << 20
        assert _same(c.reads_hdist_best2(s, read_len, k, queries), want)
        assert _same(c.reads_hdist_best2_packed(words, read_len, count, k, queries), want)
        one = c.reads_hdist_best2(s, read_len, k, int(queries[1]))  # a scalar query: Q = 1, no runner-up
        assert _same(one, r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries[1:2])) and (one[5] == 0xFF).all()
        m = 1000  # 3.8 * 10^5 pairs: the same call stays on the host
        assert _same(c.reads_hdist_best2(s[:m * read_len], read_len, k, queries), tuple(a[:m] for a in want))
        b = s.copy()
        b[s.size - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_hdist_best2(b, read_len, k, queries)
        assert (ei.value.byte, ei.value.index) == (ord("N"), s.size - 5)
        del ei
        assert _same(c.reads_hdist_best2(s, read_len, k, queries), want)  # the next call is clean
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """900,000 reads of 150 bases: the ASCII form's chunks are 894,784 whole reads (128 Mi bytes / 150), the packed form's 838,860 (4 Mi words / 5);
    no read is split, so the reads on both sides of each boundary -- which hold a planted winner and a planted runner-up each, at their first and
    last windows -- get their own two answers.  Then an N past the boundary reports its absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    read_len, count, k = 150, 900_000, 25
    per_ascii, per_packed = (128 << 20) // read_len, ((128 << 20) // 32) // 5
    assert per_packed < per_ascii < count
    queries = ro.random_queries(rng, 3, k)
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    near = [q.copy() for q in qc]
    for q in near:
        q[11] ^= 1
    for per in (per_ascii, per_packed):
        codes[per - 1, read_len - k:] = qc[0]  # the last window of the chunk's last read: the winner; its runner-up at the first window
        codes[per - 1, :k] = near[2]
        codes[per, :k] = qc[1]                 # the first window of the next chunk's first read: the winner; its runner-up at the last window
        codes[per, read_len - k:] = near[0]
        codes[per + 1, 60:60 + k] = qc[2]
        codes[per + 1, 100:100 + k] = near[1]
    s = ro.LUT[codes.reshape(-1)]
    del codes
    want = r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)
    for per in (per_ascii, per_packed):
        assert [_row(want, r) for r in (per - 1, per, per + 1)] == [(0, read_len - k, 0, 2, 0, 1), (1, 0, 0, 0, read_len - k, 1), (2, 60, 0, 1, 100, 1)]
    got = ctx.reads_hdist_best2(s, read_len, k, queries)
    assert _same(got, want), _diff(got, want)
    words = ctx.encode_fixed(s, read_len).reshape(-1)  # (the library's own fixed-length encoder: zero pad bits)
    assert np.array_equal(words[:50], ro.pack_reads(s, read_len, 10, junk=False))
    got = ctx.reads_hdist_best2_packed(words, read_len, count, k, queries)
    assert _same(got, want), _diff(got, want)
    bad_at = per_ascii * read_len + 99
    s[bad_at] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.reads_hdist_best2(s, read_len, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
    del ei


# ---- 13. seeded differential fuzz ------------------------------------------------------------------------------------------------------------
def test_seeded_differential_fuzz(ctx, oracle):
    rng = np.random.default_rng(0xF023)
    for it in range(150):
        k = int(rng.integers(1, 33))
        read_len = int(rng.integers(k, 401))
        count = int(rng.integers(1, (3001, 300, 40, 300)[it % 4]))  # up to 3000 reads, most cases smaller
        nq = int(rng.integers(1, 41))
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        want = r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)
        _check(ctx, s, read_len, count, k, queries, want, int(rng.integers(0, 16)), int(rng.integers(0, 2)), tag=(it, k, read_len, count, nq))
