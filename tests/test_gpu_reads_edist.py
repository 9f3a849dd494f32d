"""GPU tests of the indel-tolerant anchored match per read (bitnuc_reads_edist_anchored[_packed]_async, the pattern twins and the host forms above the
cutoff; scan_edist_device.h) against tests/reads_edist_oracle.py (the plain DP).  One read per lane, a wave of 64 lanes, a bounded grid walked at its
stride; a lane runs kEdistInterleave = 4 queries side by side and the remainder of Q as groups of 2 and 1; a span is four registers of 16 bases; the
ASCII form loads the aligned dwords of its span, the packed form the one to three words that hold it.  So: counts around the wave and one beyond the
bounded grid; k in {1, 2, 15, 16, 17, 31, 32} with n in {k, k + 1, 31, 32, 33, 63, 64}; packed spans inside one word and across one and two
boundaries; read lengths that give every byte residue of a span's first byte; Q around the interleave factor (u m - 1, u m, u m + 1) and the limit;
start, interior and 3' anchors, clamped and empty ranges; the planted indel, tie, duplicate, all-N, empty-set and singleton cases of the host test;
NULL second pointers; argument errors; invalid bytes inside and outside the spans; a hipGraph replay; a queue mixed with reads_hdist_anchored_async; the
host forms in one chunk and across two; the bitnuc.hpp methods; a seeded differential fuzz whose inputs are required to hold indels.  ASCII at byte
offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte and 8-mod-16 offsets with junk pad bits run on the same data.  Every
comparison is exact equality of all written arrays; guard words and bytes surround all six outputs and both dist arrays start at odd byte offsets."""
import numpy as np
import pytest

import pattern_oracle as po
import reads_anchored_oracle as ra
import reads_best_oracle as ro
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
OFFS = (0, 1, 7, 15)
U = 4  # kEdistInterleave (bitnuc_amd/csrc/edist_step_device.h)


def _dev_queries(queries, pattern=False):
    import torch
    if pattern:
        return torch.from_numpy(rp.as_patterns(queries).view(np.int32).copy()).to("cuda:0")
    return torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


class Out:
    """`triples` x (query / end with GUARD words before and after [0, count); dist inside a guarded buffer, starting at an odd byte)"""

    def __init__(self, count, triples=2):
        import torch
        self.count = count
        self.w = [torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(2 * triples)]
        self.d = [torch.full((off + count + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0") for off in DOFFS[:triples]]

    def ptrs(self, triples=None):
        out = []
        for j, d in enumerate(self.d[:triples]):
            out += [self.w[2 * j].data_ptr() + 4 * GUARD, self.w[2 * j + 1].data_ptr() + 4 * GUARD, d.data_ptr() + DOFFS[j]]
        return out

    def reset(self):
        for a in self.w:
            a.fill_(FILL32)
        for a in self.d:
            a.fill_(0x5A)

    def untouched(self, triples=(0, 1)):
        return all(bool((self.w[2 * j + i] == FILL32).all()) for j in triples for i in (0, 1)) and all(bool((self.d[j] == 0x5A).all()) for j in triples)

    def read(self, ctx=None):
        if ctx is not None:
            ctx.sync()
        n = self.count
        out = []
        for j, d in enumerate(self.d):
            for a in self.w[2 * j:2 * j + 2]:
                a = a.cpu().numpy().view(np.uint32)
                assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / end written outside [0, count)"
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


def _both(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=0, woff=0, words=None, pattern=False):
    """(six arrays of the ASCII form, six of the packed form), guards checked"""
    import torch
    nq = len(queries)
    t, ptr = _ascii_dev(s, off)
    w = ro.pack_reads(s, read_len, count) if words is None else words
    tw, wptr = _words_dev(w, woff)
    dq = _dev_queries(queries, pattern)
    o1, o2 = Out(count), Out(count)
    fa, fp = (ctx.reads_pattern_edist_anchored_async, ctx.reads_pattern_edist_anchored_packed_async) if pattern else \
             (ctx.reads_edist_anchored_async, ctx.reads_edist_anchored_packed_async)
    torch.cuda.synchronize()
    fa(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=pos_lo, pos_hi=pos_hi)
    fp(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=pos_lo, pos_hi=pos_hi)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, want=None, off=0, woff=0, words=None, tag=(), pattern=False):
    if want is None:
        want = (eo.reads_pattern_edist if pattern else eo.reads_edist)(s, read_len, count, k, queries, pos_lo, pos_hi)
    a, p = _both(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off, woff, words, pattern)
    assert _same(a, want), ("ascii", tag, _diff(a, want))
    assert _same(p, want), ("packed", tag, _diff(p, want))
    return want


def _random(rng, read_len, count, k, nq, pos_lo=None, n=None, lower=True):
    """random queries and reads; with a span given, about half of the reads carry a query with 0 .. 3 edits inside it"""
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    if n is not None:
        for r in rng.choice(count, size=min(count, 64, (count + 1) // 2), replace=False):
            c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, nq))], k), int(rng.integers(0, 4)))[:n]
            at = int(r) * read_len + pos_lo + int(rng.integers(0, n - len(c) + 1))
            s[at:at + len(c)] = ro.LUT[c]
    if lower:
        s[rng.random(s.size) < 0.3] |= 0x20
    return queries, s


def _span(read_len, k, n, where):
    """(pos_lo, pos_hi) of a span of n bases: at the start, in the interior, at the 3' end (pos_hi = to the end), and clamped by the read's end"""
    lo = (0, (read_len - n) // 2, read_len - n, read_len - n)[where]
    return lo, (lo + n - k, lo + n - k, None, read_len + 5)[where]


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 63, 64, 65, 255, 257))
def test_counts_around_the_wave_and_the_block(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, read_len, nq, n) in enumerate(((16, 150, 9, 19), (31, 65, 3, 41), (5, 33, 33, 5))):
        for where in range(4):
            pos_lo, pos_hi = _span(read_len, k, n, where)
            queries, s = _random(rng, read_len, count, k, nq, pos_lo, n)
            _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=OFFS[(i + where + count) % 4], woff=(i + count) % 2, tag=(count, k, read_len, pos_lo, pos_hi))


def test_a_count_beyond_the_bounded_grid(ctx):
    """more reads than the grid has lanes (at most 8 workgroups of 256 lanes per CU): some lanes walk two reads"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 4161
    rng = np.random.default_rng(5)
    k, read_len, nq, n = 6, 21, 3, 9
    queries, s = _random(rng, read_len, count, k, nq, 12, n)
    _check(ctx, s, read_len, count, k, queries, 12, None, off=1, woff=1)


@pytest.mark.parametrize("k", (1, 2, 15, 16, 17, 31, 32))
def test_k_and_spans_around_the_registers(ctx, k):
    """n in {k, k + 1, 31, 32, 33, 63, 64}: a span ends inside, at the end of and just behind a register of 16 bases; read lengths 150 .. 153 put a span's
    first byte at every residue mod 4"""
    rng = np.random.default_rng(300 + k)
    for i, n in enumerate(sorted({k, k + 1, 31, 32, 33, 63, 64})):
        if n < k:
            continue
        read_len, count, nq = 150 + (i + k) % 4, 70, (1, 2, 3, 5, 7, 8, 9)[i % 7]
        pos_lo, pos_hi = _span(read_len, k, n, (i + k) % 4)
        queries, s = _random(rng, read_len, count, k, nq, pos_lo, n)
        _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=OFFS[i % 4], woff=i % 2, tag=(k, n, read_len, pos_lo, pos_hi, nq))


@pytest.mark.parametrize("nq", (1, 2, 3, 4, 5, 7, 8, 9, 33, 3 * U - 1, 3 * U, 3 * U + 1))
def test_queries_around_the_interleave_factor(ctx, nq):
    rng = np.random.default_rng(400 + nq)
    k, read_len, count, n = 16, 150, 130, 23
    queries, s = _random(rng, read_len, count, k, nq, read_len - n, n)
    if nq >= 2:
        queries[nq - 1] = queries[0] ^ (np.uint64(1) << np.uint64(63))  # the last query of the last group: an equal duplicate of query 0
    _check(ctx, s, read_len, count, k, queries, read_len - n, None, off=OFFS[nq % 4], woff=nq % 2, tag=nq)
    _check(ctx, s, read_len, count, k, rp.singletons(queries, k), read_len - n, None, off=OFFS[nq % 4], woff=nq % 2, tag=nq, pattern=True)


def test_read_lengths_that_give_every_byte_residue(ctx):
    rng = np.random.default_rng(17)
    for read_len in (61, 62, 63, 64):
        for pos_lo in (0, 1, 2, 3):
            k, count, nq, n = 11, 67, 5, 17
            queries, s = _random(rng, read_len, count, k, nq, pos_lo, n)
            _check(ctx, s, read_len, count, k, queries, pos_lo, pos_lo + n - k, off=OFFS[(read_len + pos_lo) % 4], tag=(read_len, pos_lo))


def test_packed_spans_inside_a_word_and_across_one_and_two_boundaries(ctx):
    rng = np.random.default_rng(23)
    read_len, count, k, nq = 150, 66, 9, 6
    for pos_lo, n in ((0, 32), (3, 20), (32, 32), (64, 9), (20, 20), (31, 2 + k), (63, 33), (10, 64), (30, 40), (31, 34), (63, 64), (86, 64), (95, 50)):
        queries, s = _random(rng, read_len, count, k, nq, pos_lo, n)
        for woff in (0, 1):
            _check(ctx, s, read_len, count, k, queries, pos_lo, pos_lo + n - k, woff=woff, tag=(pos_lo, n))


def test_empty_ranges_and_fills(ctx):
    import torch
    rng = np.random.default_rng(31)
    read_len, count = 40, 70
    queries, s = _random(rng, read_len, count, 8, 3)
    for k, qq, pos_lo, pos_hi in ((0, queries, 0, None), (41, queries, 0, None), (8, queries[:0], 0, 3), (8, queries, 33, None), (8, queries, 5, 4), (8, queries, 2**40, None)):
        want = eo.reads_edist(s, read_len, count, k, qq, pos_lo, pos_hi)
        assert _same(want, eo.fill6(count))
        if k <= 32:
            _check(ctx, s, read_len, count, k, qq, pos_lo, pos_hi, want, off=1, woff=1, tag=(k, pos_lo, pos_hi))
    o = Out(count)  # count == 0: nothing written
    t, ptr = _ascii_dev(s, 0)
    torch.cuda.synchronize()
    ctx.reads_edist_anchored_async(ptr, read_len, 0, 8, _dev_queries(queries), 3, *o.ptrs(), pos_lo=0, pos_hi=3)
    ctx.sync()
    assert o.untouched()


# ---- 2. planted cases (those of tests/test_reads_edist_host.py) -------------------------------------------------------------------------------
def test_planted_indels_by_hand(ctx):
    k, read_len, lo, n, s, queries = eo.planted_cases()
    want = _check(ctx, s, read_len, 5, k, queries, lo, lo + n - k, off=7, woff=1)
    assert [list(want[i]) for i in range(3)] == [[1] * 5, [29, 31, 30, 30, 30], [1, 1, 1, 2, 0]]
    _check(ctx, s, read_len, 5, k, rp.singletons(queries, k), lo, lo + n - k, want, off=1, pattern=True)
    ham = ra.reads_anchored(s, read_len, 5, k, queries, lo, lo + n - k)
    assert (want[2] <= ham[2]).all() and (want[2][:2] < ham[2][:2]).all()


def test_ties_two_ends_two_queries_and_a_duplicate(ctx):
    k, read_len = 6, 40
    q = np.array([0, 1, 2, 3, 1, 0])
    codes = np.full(read_len, 2)
    codes[5:11], codes[20:26] = q, q
    s = np.tile(ro.LUT[codes].astype(np.uint8), 3)
    far = ro.word_of([3] * k)
    queries = np.array([far, ro.word_of(q), far, ro.word_of(q) | (1 << 40), far], dtype=np.uint64)
    want = _check(ctx, s, read_len, 3, k, queries, 0, None, off=15)
    assert tuple(int(a[1]) for a in want) == (1, 11, 0, 3, 11, 0)  # the smaller end; the equal duplicate at the same distance and end
    near = q.copy()
    near[2] = 0
    queries = np.array([ro.word_of(near), far, ro.word_of(near)], dtype=np.uint64)
    want = _check(ctx, s, read_len, 3, k, queries, 0, None, woff=1)
    assert tuple(int(a[2]) for a in want) == (0, 11, 1, 2, 11, 1)  # two queries at the same distance: the smaller index
    want = _check(ctx, s, read_len, 3, k, queries[:1], 0, None)
    assert tuple(int(a[0]) for a in want) == (0, 11, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF)  # one query: the fill in the second triple


@pytest.mark.parametrize("k,read_len,lo,hi", ((1, 20, 3, 9), (12, 50, 7, 30), (32, 150, 86, None)))
def test_patterns_all_n_empty_set_and_singletons(ctx, k, read_len, lo, hi):
    rng = np.random.default_rng(0x9A7 + k)
    count = 77
    queries, s = _random(rng, read_len, count, k, 5)
    exact = _check(ctx, s, read_len, count, k, queries, lo, hi, off=1)
    sing = rp.singletons(queries, k)
    _check(ctx, s, read_len, count, k, sing, lo, hi, exact, off=7, woff=1, pattern=True)  # byte for byte the exact form
    all_n = po.from_iupac("N" * k)
    want = _check(ctx, s, read_len, count, k, [all_n, sing[0]], lo, hi, pattern=True)
    assert (want[0] == 0).all() and (want[1] == lo + k).all() and (want[2] == 0).all()
    sets = [po.random_sets(rng, k) for _ in range(6)]
    sets[2] = [set() if i == k // 2 else x for i, x in enumerate(sets[2])]
    sets[5] = [set()] * k  # matches nothing: distance k at the first end
    pats = rp.as_patterns([po.from_sets(x) for x in sets])
    _check(ctx, s, read_len, count, k, pats, lo, hi, off=15, pattern=True)
    want = _check(ctx, s, read_len, count, k, pats[5:], lo, hi, pattern=True)
    assert (want[2] == k).all() and (want[1] == lo + 1).all()


def test_never_above_the_hamming_form(ctx):
    rng = np.random.default_rng(0xBEE)
    k, read_len, count, nq, lo = 16, 150, 300, 12, 130
    queries, s = _random(rng, read_len, count, k, nq, lo, 20)
    want = _check(ctx, s, read_len, count, k, queries, lo, None)
    ham = ra.reads_anchored(s, read_len, count, k, queries, lo, None)
    assert (want[2] <= ham[2]).all() and (want[2] < ham[2]).any()


# ---- 3. the contract --------------------------------------------------------------------------------------------------------------------------
def test_null_second_pointers_write_the_best_triple_only(ctx):
    import torch
    rng = np.random.default_rng(9)
    read_len, count, k, nq = 65, 99, 13, 10
    queries, s = _random(rng, read_len, count, k, nq, 2, 18)
    want = eo.reads_edist(s, read_len, count, k, queries, 2, 7)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(ro.pack_reads(s, read_len, count), 1)
    dq = _dev_queries(queries)
    for fn, src in ((ctx.reads_edist_anchored_async, ptr), (ctx.reads_edist_anchored_packed_async, wptr)):
        o = Out(count)
        torch.cuda.synchronize()
        fn(src, read_len, count, k, dq, nq, *o.ptrs(1), pos_lo=2, pos_hi=7)
        ctx.sync()
        assert o.untouched(triples=(1,)) and _same(o.read()[:3], want[:3])


def _raw_err(fn, src, read_len, count, k, dq, nq, six, pos_lo, pos_hi):
    """(kind, value) of the error a device call raises, through the raw entry point (the Python error carries no value for Unsupported)"""
    import ctypes as C
    from bitnuc_amd import _lib as L
    ctx = fn.__self__
    raw = getattr(L.load(), "bitnuc_" + fn.__name__)
    err = L.BitnucErr()
    st = raw(ctx._h, C.c_void_p(src), read_len, count, k, pos_lo, C.c_size_t(-1).value if pos_hi is None else pos_hi, C.c_void_p(dq.data_ptr()), nq,
             *(C.c_void_p(p) for p in six), C.byref(err))
    return ({L.UNSUPPORTED: "Unsupported", L.OK: "OK"}.get(st, st), int(err.value))


def test_argument_errors_leave_the_outputs_untouched(ctx):
    import torch
    import bitnuc_amd as bn
    s = ro.LUT[np.random.default_rng(2).integers(0, 4, size=15000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(ro.pack_reads(s, 150, 100), 0)
    dq = _dev_queries(np.zeros(32, dtype=np.uint64))  # sixteen patterns as well
    o = Out(100)
    six = o.ptrs()
    torch.cuda.synchronize()
    for fn, src in ((ctx.reads_edist_anchored_async, ptr), (ctx.reads_edist_anchored_packed_async, wptr), (ctx.reads_pattern_edist_anchored_async, ptr),
                    (ctx.reads_pattern_edist_anchored_packed_async, wptr)):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 150, 100, 33, dq, 65537, *six, pos_lo=0, pos_hi=100)  # k first
        assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
        assert _raw_err(fn, src, 150, 100, 12, dq, 65537, six, 0, 100) == ("Unsupported", 65537)  # then the query count, before the span
        for pos_lo, pos_hi, span in ((0, 53, 65), (0, None, 150), (80, None, 70)):
            assert _raw_err(fn, src, 150, 100, 12, dq, 16, six, pos_lo, pos_hi) == ("Unsupported", span)
        for bad in ((six[0], six[1], six[2], 0, six[4], six[5]), (six[0], six[1], six[2], six[3], 0, 0), (six[0], six[1], six[2], six[3] + 2, six[4], six[5]),
                    (six[0], 0, six[2], six[3], six[4], six[5])):
            with pytest.raises(bn.NucleotideError) as ei:
                fn(src, 150, 100, 12, dq, 16, *bad, pos_lo=0, pos_hi=3)
            assert ei.value.kind == "Unsupported"
        del ei
    with pytest.raises(bn.NucleotideError):
        ctx.reads_edist_anchored_packed_async(wptr + 4, 150, 100, 12, dq, 16, *six, pos_lo=0, pos_hi=3)  # words not 8-byte aligned
    ctx.sync()
    assert o.untouched()


def test_invalid_bytes_inside_and_outside_the_spans(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, read_len, count, nq, lo, hi = 17, 150, 400, 9, 129, None  # the spans: bytes 129 .. 149 of every read
    queries, s = _random(rng, read_len, count, k, nq, lo, 21)
    want = eo.reads_edist(s, read_len, count, k, queries, lo, hi)
    dq = _dev_queries(queries)
    b = s.copy()
    b[0], b[128], b[150 * 7 + 5], b[150 * 399 + 128] = ord("N"), ord("n"), 0, 0xFF  # outside every span
    for off in (0, 3):
        t, ptr = _ascii_dev(b, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_anchored_async(ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o.read(ctx), want)  # no error, correct results
    for bad_at, off in ((150 * 200 + 129, 0), (150 * 0 + 149, 9), (150 * 399 + 140, 5)):  # a span's first byte, read 0's last, the last read
        c = b.copy()
        c[bad_at] = ord("N")
        if bad_at + 150 * 3 < c.size:
            c[bad_at + 150 * 3] = ord("x")  # a later one, in another read: the first in buffer order wins
        t, ptr = _ascii_dev(c, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_anchored_async(ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing is left for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean and correct
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_anchored_async(ptr2, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o.read(ctx), want)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries on one read are accepted (the winner planted at the last index, its duplicate in the middle), one more is refused"""
    rng = np.random.default_rng(65537)
    k, read_len, count, nq = 20, 28, 1, 65536  # (k = 20: no random query comes within one edit of the read)
    queries = ro.random_queries(rng, nq, k)
    queries[30000] = queries[nq - 1] ^ (np.uint64(1) << np.uint64(60))
    codes = rng.integers(0, 4, size=read_len)
    codes[5:5 + k - 1] = np.delete(ro.query_codes(queries[nq - 1], k), 4)  # the last query with one base deleted
    s = ro.LUT[codes].astype(np.uint8)
    want = _check(ctx, s, read_len, count, k, queries, 2, None, off=1, woff=1)
    assert tuple(int(a[0]) for a in want) == (30000, 5 + k - 1, 1, nq - 1, 5 + k - 1, 1)
    o = Out(1)
    t, ptr = _ascii_dev(s, 0)
    dq = _dev_queries(np.zeros(nq + 1, dtype=np.uint64))
    assert _raw_err(ctx.reads_edist_anchored_async, ptr, read_len, count, k, dq, nq + 1, o.ptrs(), 2, None) == ("Unsupported", nq + 1)
    ctx.sync()
    assert o.untouched()


def test_graph_replay_after_the_reads_and_the_queries_changed():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    read_len, count, k, nq, lo, hi = 151, 2000, 31, 9, 0, 3
    (q1, s1), (q2, s2) = _random(rng, read_len, count, k, nq, lo, 34), _random(rng, read_len, count, k, nq, lo, 34)
    want1, want2 = eo.reads_edist(s1, read_len, count, k, q1, lo, hi), eo.reads_edist(s2, read_len, count, k, q2, lo, hi)
    assert not np.array_equal(want1[0], want2[0]) and not np.array_equal(want1[3], want2[3])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = ro.pack_reads(s1, read_len, count)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        o1, o2 = Out(count), Out(count)
        c.reads_edist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi)  # warm-up outside the capture: sizes the scratch
        c.reads_edist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.reads_edist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi)
                c.reads_edist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi)
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


def test_mixed_queue_with_one_sync(ctx):
    """the edit-distance calls (ASCII, packed and pattern forms in turn) between reads_hdist_anchored_async calls on one context, different (count,
    n_queries) between consecutive calls (both lay out scratch 10 anew), one sync at the end, every result checked afterwards"""
    import torch
    rng = np.random.default_rng(809)
    k, read_len = 21, 150
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (800, 3))):  # inputs and outputs first
        lo, hi = ((0, 3), (126, None), (60, 80))[i % 3]
        queries, s = _random(rng, read_len, count, k, nq, lo, 24, lower=False)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         dp=_dev_queries(rp.singletons(queries, k), True), out=Out(count), ham=Out(count), wdev=_words_dev(ro.pack_reads(s, read_len, count), i & 1),
                         rng=(lo, hi)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, ptr, dq, (lo, hi) = j["i"], j["count"], j["nq"], j["ascii"][1], j["dq"], j["rng"]
        if i % 4 == 0:
            ctx.reads_edist_anchored_async(ptr, read_len, count, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        elif i % 4 == 1:
            ctx.reads_edist_anchored_packed_async(j["wdev"][1], read_len, count, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        elif i % 4 == 2:
            ctx.reads_pattern_edist_anchored_async(ptr, read_len, count, k, j["dp"], nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        else:
            ctx.reads_pattern_edist_anchored_packed_async(j["wdev"][1], read_len, count, k, j["dp"], nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *j["ham"].ptrs(), pos_lo=lo, pos_hi=hi)
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, count, nq, s, queries, (lo, hi) = j["i"], j["count"], j["nq"], j["s"], j["queries"], j["rng"]
        want = eo.reads_edist(s, read_len, count, k, queries, lo, hi)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        ham = j["ham"].read()
        assert _same(ham, ra.reads_anchored(s, read_len, count, k, queries, lo, hi)), i
        assert (got[2] <= ham[2]).all()


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """900,000 reads of 150 bases, a span of 12 bases at the 3' end, two queries (21.6 * 10^6 span-base-query pairs, above the default cutoff of 2^20) on
    a context with the default dispatch: the ASCII form's chunks are 894,784 whole reads (128 Mi bytes / 150), the packed form's 838,860 (4 Mi words /
    5); the reads on both sides of each boundary hold a planted winner.  100,000 reads run in one chunk, 20,000 stay on the host.  Then an N past the
    boundary, inside a span, reports its absolute index; one outside the spans is ignored."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    read_len, count, k, w = 150, 900_000, 9, 3
    lo = read_len - k - w
    per_ascii, per_packed = (128 << 20) // read_len, ((128 << 20) // 32) // 5
    assert per_packed < per_ascii < count
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    for per in (per_ascii, per_packed):
        codes[per - 1, lo + 3:] = qc[0]                          # the chunk's last read: query 0 at the read's end
        codes[per, lo:lo + k] = qc[1]                            # the next chunk's first read: query 1 at the span's start
        codes[per + 1, lo + 1:lo + k] = np.delete(qc[0], 4)      # query 0 with one base deleted
    s = ro.LUT[codes.reshape(-1)]
    del codes
    want = eo.reads_edist(s, read_len, count, k, queries, lo, None)
    for per in (per_ascii, per_packed):
        assert [tuple(int(a[r]) for a in want[:3]) for r in (per - 1, per)] == [(0, read_len, 0), (1, lo + k, 0)] and int(want[2][per + 1]) <= 1
    c = bn.Context(0)
    try:
        got = c.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo)
        assert _same(got, want), _diff(got, want)
        words = c.encode_fixed(s, read_len).reshape(-1)
        got = c.reads_edist_anchored_packed(words, read_len, count, k, queries, pos_lo=lo)
        assert _same(got, want), _diff(got, want)
        got = c.reads_pattern_edist_anchored_packed(words, read_len, count, k, rp.singletons(queries, k), pos_lo=lo)
        assert _same(got, want), _diff(got, want)
        m, big = 20_000, 100_000  # 480,000 pairs: the host; 2.4 * 10^6 pairs: one chunk through the device
        assert m * 12 * 2 < 1 << 20 <= big * 12 * 2
        assert _same(c.reads_edist_anchored(s[:big * read_len], read_len, k, queries, pos_lo=lo), tuple(a[:big] for a in want))
        assert _same(c.reads_edist_anchored_packed(words[:big * 5], read_len, big, k, queries, pos_lo=lo, second=False), tuple(a[:big] for a in want[:3]))
        assert _same(c.reads_edist_anchored(s[:m * read_len], read_len, k, queries, pos_lo=lo), tuple(a[:m] for a in want))  # stays on the host
        s[per_ascii * read_len + 7] = ord("N")  # outside the spans: ignored
        assert _same(c.reads_pattern_edist_anchored(s, read_len, k, rp.singletons(queries, k), pos_lo=lo), want)
        bad_at = per_ascii * read_len + lo + 9
        s[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
    finally:
        c.close()


def test_cpp_mirror_of_the_edist_forms(ctx, tmp_path):
    """the four reads_*edist_anchored* methods of include/bitnuc.hpp against the plain DP, via tests/cpp/test_reads_edist_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_reads_edist_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_reads_edist_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_seeded_differential_fuzz(ctx):
    """200 small cases.  In each at least half of the reads carry a copy of one of the queries with 0 .. 3 random edits, at least one of them an indel
    (the first planted read of a case: exactly one deletion or insertion).  On the oracles alone: in at least a quarter of a case's reads the edit
    distance is strictly below the anchored Hamming distance -- a condition on the INPUTS, so that substitution-only data cannot pass for a test of this
    kernel.  (k >= 8 and a span of at least k + 2 bases, so that an indel costs the Hamming form several mismatches and the planted copy fits.)"""
    rng = np.random.default_rng(0xED17)
    for it in range(200):
        k = int(rng.integers(8, 33))
        n = int(rng.integers(k + 2, min(64, k + 12) + 1))
        read_len = int(rng.integers(n, 161))
        count = int(rng.integers(4, (300, 130, 40, 70)[it % 4]))
        nq = int(rng.integers(1, 14))
        kind = it % 4
        pos_lo = 0 if kind == 0 else (read_len - n if kind == 1 else int(rng.integers(0, read_len - n + 1)))
        pos_hi = None if kind == 1 else pos_lo + n - k
        queries = ro.random_queries(rng, nq, k)
        codes = rng.integers(0, 4, size=(count, read_len))
        for j, r in enumerate(rng.choice(count, size=(count + 1) // 2 + count // 4, replace=False)):
            edits = 1 if j == 0 else int(rng.integers(1, 4))
            c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, nq))], k), edits)[:n]
            at = int(rng.integers(0, n - len(c) + 1))
            codes[r, pos_lo + at:pos_lo + at + len(c)] = c
        s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
        s[rng.random(s.size) < 0.3] |= 0x20
        want = eo.reads_edist(s, read_len, count, k, queries, pos_lo, pos_hi)
        ham = ra.reads_anchored(s, read_len, count, k, queries, pos_lo, pos_hi)
        assert (want[2] <= ham[2]).all()
        assert 4 * int((want[2] < ham[2]).sum()) >= count, (it, k, n, count, int((want[2] < ham[2]).sum()))  # the inputs hold indels
        _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, want, off=int(rng.integers(0, 16)), woff=int(rng.integers(0, 2)),
               tag=(it, k, read_len, count, nq, pos_lo, pos_hi))
