"""GPU tests of the anchored best match and runner-up per read (bitnuc_reads_hdist_anchored[_packed]_async and the host forms above the cutoff;
scan_anchored_device.h) against tests/reads_anchored_oracle.py.  The tile is 32 reads x 32 (query, offset) rows, a wave takes 64 reads at a time, K-steps
end at 16 bases: counts around 32 / 64 and beyond the bounded grid, (queries, offsets) with rows per query of 1 .. 64 and queries astride tiles, k and
spans around the K-steps, read lengths that give every byte residue and packed spans inside one word and across one or two word boundaries; start,
interior and 3' anchors, clamped and empty ranges; planted cases for the range, the runner-up, ties, duplicates and matches astride two reads; the
identities with reads_hdist_best2*_async; NULL second pointers; argument errors; invalid bytes inside and outside the spans; the query limit; a hipGraph
replay; a queue of mixed calls; the host forms in one chunk and across two; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 / +15 with
lowercase bases and packed words at 16-byte and 8-mod-16 offsets with junk pad bits run on the same data.  Every comparison is exact equality of all
written arrays; guard words and bytes surround all six outputs and both dist arrays start at odd byte offsets."""
import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_anchored_oracle as ra

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
NO = ro.NO_U32
OFFS = (0, 1, 7, 15)


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


def _row(want, r):
    return tuple(int(a[r]) for a in want)


def _both(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=0, woff=0, words=None):
    """(six arrays of the ASCII form, six of the packed form), guards checked"""
    import torch
    nq = len(queries)
    t, ptr = _ascii_dev(s, off)
    w = ro.pack_reads(s, read_len, count) if words is None else words
    tw, wptr = _words_dev(w, woff)
    dq = _dev_queries(queries)
    o1, o2 = Out(count), Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=pos_lo, pos_hi=pos_hi)
    ctx.reads_hdist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=pos_lo, pos_hi=pos_hi)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, want=None, off=0, woff=0, words=None, tag=()):
    if want is None:
        want = ra.reads_anchored(s, read_len, count, k, queries, pos_lo, pos_hi)
    a, p = _both(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off, woff, words)
    assert _same(a, want), ("ascii", tag, _diff(a, want))
    assert _same(p, want), ("packed", tag, _diff(p, want))
    return want


def _random(rng, read_len, count, k, nq, lower=True):
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    if lower:
        s[rng.random(s.size) < 0.3] |= 0x20
    return queries, s


def _anchors(read_len, k, offsets):
    """(pos_lo, pos_hi) with `offsets` admissible offsets (as far as the read allows): the start, an interior range, the 3' end (pos_hi = to the end),
    and pos_hi beyond the read's end (clamped)"""
    last = read_len - k
    w = min(offsets, last + 1)
    return sorted({(0, w - 1), ((last + 1 - w) // 2, (last + 1 - w) // 2 + w - 1), (last + 1 - w, None), (last + 1 - w, last + 9)}, key=str)


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 31, 32, 33, 63, 65, 2049))
def test_counts_around_the_tile_and_the_wave(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, read_len, nq, offsets) in enumerate(((16, 150, 17, 4), (31, 65, 3, 11), (5, 33, 33, 1))):
        queries, s = _random(rng, read_len, count, k, nq)
        for pos_lo, pos_hi in _anchors(read_len, k, offsets):
            _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=OFFS[(i + count) % 4], woff=(i + count) % 2, tag=(count, k, read_len, pos_lo, pos_hi))


def test_a_count_beyond_the_bounded_grid(ctx):
    """more blocks of 64 reads than the grid has waves (at most 4 workgroups of four waves per CU): some waves loop"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 4 * 64 + 4161
    rng = np.random.default_rng(5)
    k, read_len, nq = 12, 33, 5
    queries, s = _random(rng, read_len, count, k, nq)
    _check(ctx, s, read_len, count, k, queries, 18, None, off=1, woff=1)


@pytest.mark.parametrize("nq,offsets,k", ((1, 1, 16), (1, 33, 32), (31, 1, 16), (32, 1, 16), (33, 1, 16), (3, 11, 21), (17, 4, 16), (257, 4, 16), (5, 16, 9),
                                         (6, 17, 9), (7, 32, 22), (3, 64, 1), (9, 40, 2), (70, 2, 15), (11, 8, 17)))
def test_queries_and_offsets_around_the_tile(ctx, nq, offsets, k):
    """rows per query of 1, 2, 4, 8, 16 (several queries per lane), 32 (a query per tile) and 64 (a query per two tiles); 3 x 11 -> 3 x 16 rows: a query
    astride the two lanes of a read; the last tile partly empty"""
    rng = np.random.default_rng(1000 * nq + offsets)
    for read_len, count in ((150, 70), (offsets + k - 1, 33), (65, 40)):
        if read_len < offsets + k - 1:
            continue
        queries, s = _random(rng, read_len, count, k, nq)
        for pos_lo, pos_hi in _anchors(read_len, k, offsets):
            _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=OFFS[(nq + read_len) % 4], woff=nq % 2, tag=(nq, offsets, k, read_len, pos_lo, pos_hi))


@pytest.mark.parametrize("k", (1, 2, 15, 16, 17, 21, 22, 31, 32))
def test_k_and_spans_around_the_k_steps(ctx, k):
    rng = np.random.default_rng(40 + k)
    for span in sorted({k, 16, 17, 21, 22, 32, 33, 48, 49, 64}):
        if span < k:
            continue
        offsets = span - k + 1
        for read_len in sorted({k, 33, 64, 65, 150, 151}):
            if read_len < span:
                continue
            count, nq = 67, (1, 2, 5, 33)[(span + read_len) % 4]
            queries, s = _random(rng, read_len, count, k, nq)
            for pos_lo, pos_hi in _anchors(read_len, k, offsets):
                _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=OFFS[(span + k) % 4], woff=(span + read_len) % 2, tag=(k, span, read_len, pos_lo, pos_hi))


def test_packed_spans_inside_a_word_and_across_one_and_two_boundaries(ctx):
    rng = np.random.default_rng(77)
    k, read_len, count = 16, 150, 65
    queries, s = _random(rng, read_len, count, k, 6)
    for pos_lo, pos_hi in ((3, 5), (20, 20), (20, 24), (30, 70), (60, 100), (95, 95), (120, None)):
        hi, span = ra.span_of(read_len, k, pos_lo, pos_hi)
        assert span <= 64
        _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=7, woff=1, tag=(pos_lo, pos_hi))


def test_empty_ranges_and_fills(ctx):
    import torch
    rng = np.random.default_rng(3)
    queries, s = _random(rng, 40, 50, 8, 4)
    for k, read_len, nq, pos_lo, pos_hi in ((8, 40, 4, 33, None), (8, 40, 4, 5, 4), (8, 40, 4, 2**40, None), (0, 40, 4, 0, None), (8, 7, 4, 0, None), (8, 40, 0, 0, 3)):
        _check(ctx, s, read_len, 50, k, queries[:nq], pos_lo, pos_hi, want=r2.fill6(50), tag=(k, read_len, nq, pos_lo))
    t, ptr = _ascii_dev(s, 0)
    dq = _dev_queries(queries)
    o = Out(50)
    torch.cuda.synchronize()
    ctx.reads_hdist_anchored_async(ptr, 40, 0, 8, dq, 4, *o.ptrs(), pos_lo=0, pos_hi=3)  # count == 0: nothing written
    ctx.sync()
    assert o.untouched()
    one = _check(ctx, s, 40, 50, 8, queries[2:3], 30, None)  # one query: the runner-up is the fill
    assert (one[2] != 0xFF).all() and (one[3] == NO).all() and (one[4] == NO).all() and (one[5] == 0xFF).all()


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------------------------
def test_the_range_is_honoured(ctx):
    """a distance-0 copy of query 5 one base before pos_lo (even reads) or one base after hi_eff (odd reads) is not found, a distance-2 copy inside the
    range is; reads_hdist_best2_async over the whole reads finds the copies outside"""
    import torch
    rng = np.random.default_rng(51)
    k, read_len, count, nq, lo, hi = 20, 150, 70, 24, 40, 75
    queries = ro.random_queries(rng, nq, k)
    q5 = ro.query_codes(queries[5], k)
    near = q5.copy()
    near[[2, 9]] ^= 1
    codes = rng.integers(0, 4, size=(count, read_len))
    for r in range(count):
        out_at, in_at = (lo - 1, 59) if r % 2 == 0 else (hi + 1, 45)
        codes[r, out_at:out_at + k] = q5
        codes[r, in_at:in_at + k] = near
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    for r in range(count):
        assert _row(want, r)[:3] == ((5, 59, 2) if r % 2 == 0 else (5, 45, 2))
    for off, woff in ((0, 0), (7, 1), (15, 0)):
        _check(ctx, s, read_len, count, k, queries, lo, hi, want, off, woff)
    t, ptr = _ascii_dev(s, 1)
    o = Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_best2_async(ptr, read_len, count, k, _dev_queries(queries), nq, *o.ptrs())
    whole = o.read(ctx)
    for r in range(count):
        assert _row(whole, r)[:3] == ((5, lo - 1, 0) if r % 2 == 0 else (5, hi + 1, 0))


@pytest.mark.parametrize("win,run,nq", ((3, 7, 24), (3, 20, 24), (3, 300, 304), (20, 7, 24)))
def test_the_winners_second_window_is_never_the_runner_up(ctx, win, run, nq):
    """the winner at two offsets inside the range (distances 0 and 1) and another query at distance 2 (the same tile, the next, a far one; a LOWER query
    at a greater distance): the runner-up is the other query"""
    rng = np.random.default_rng(3400 + win + run)
    k, read_len, count, lo, hi = 16, 150, 40, 100, 132  # 33 offsets, span 48: room for three windows
    queries = ro.random_queries(rng, nq, k)
    qw, qr = ro.query_codes(queries[win], k), ro.query_codes(queries[run], k)
    w1, r2c = qw.copy(), qr.copy()
    w1[5] ^= 3
    r2c[[1, 6]] ^= 2
    codes = rng.integers(0, 4, size=(count, read_len))
    codes[:, 100:100 + k], codes[:, 116:116 + k], codes[:, 132:132 + k] = w1, qw, r2c
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    for r in range(count):
        assert _row(want, r) == (win, 116, 0, run, 132, 2)
    _check(ctx, s, read_len, count, k, queries, lo, hi, want, off=7, woff=1)


@pytest.mark.parametrize("orig,dup,nq", ((4, 5, 24), (1, 6, 24), (4, 9, 24), (4, 20, 24), (4, 300, 304)))
def test_ties_an_equal_query_is_the_runner_up_and_the_lower_offset_wins(ctx, orig, dup, nq):
    """equal duplicate queries, best = the first, runner-up = the duplicate at the same offset.  Four offsets: a tile holds eight queries, 0 .. 3 in the
    registers of lane l, 4 .. 7 in those of lane l ^ 32.  (4, 5): the same tile and the same lane (the in-register top-2); (1, 6): the same tile, the
    partner lane (the merge after the last tile); (4, 9): the next tile; (4, 20) and (4, 300): far tiles.  Then the query at two offsets at the same
    distance: the lower offset"""
    rng = np.random.default_rng(600 + dup)
    k, read_len, count, lo, hi = 16, 65, 37, 10, 13  # four offsets: eight queries per tile
    queries = ro.random_queries(rng, nq, k)
    queries[dup] = queries[orig] ^ (np.uint64(1) << np.uint64(63))
    q4 = ro.query_codes(queries[orig], k)
    one = q4.copy()
    one[3] ^= 1
    codes = rng.integers(0, 4, size=(count, read_len))
    codes[:, 11:11 + k] = one
    codes[::2, 13:13 + k] = one  # even reads: distance 1 at offsets 11 and 13 -- unless the overlap makes 11 differ: the oracle decides, see below
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    for r in range(1, count, 2):
        assert _row(want, r) == (orig, 11, 1, dup, 11, 1)
    assert (want[0] == orig).all() and (want[3] == dup).all() and (want[1] == want[4]).all()
    _check(ctx, s, read_len, count, k, queries, lo, hi, want, off=1, woff=0)
    # an exact tie between two offsets of one query: poly-A reads and a poly-A query
    queries[0] = 0
    s = np.full(count * read_len, ord("A"), dtype=np.uint8)
    want = _check(ctx, s, read_len, count, k, queries, lo, hi, off=15, woff=1)
    assert _row(want, 5)[:3] == (0, lo, 0)


@pytest.mark.parametrize("read_len", (33, 150))
def test_a_match_that_straddles_two_reads_is_seen_by_neither_triple(ctx, read_len):
    """the last bases of read r and the first of read r + 1 spell query 3 (range at the 3' end); the packed pad bits hold the completing bases"""
    rng = np.random.default_rng(88 + read_len)
    k, count, nq, w = 12, 66, 6, 3
    queries = ro.random_queries(rng, nq, k)
    q3 = ro.query_codes(queries[3], k)
    codes = rng.integers(0, 4, size=(count, read_len))
    for r in range(count - 1):
        cut = 5 + r % 3  # the read's last `cut` bases are the query's first
        codes[r, read_len - cut:] = q3[:cut]
        codes[r + 1, :k - cut] = q3[cut:]
    s = ro.LUT[codes.reshape(-1)].astype(np.uint8)
    words = ro.pack_reads(s, read_len, count, junk=False)
    wpr = (read_len + 31) // 32
    for r in range(count - 1):  # the pad bits of read r: the bases that would complete the match
        cut, pad = 5 + r % 3, 32 * wpr - read_len
        for i, c in enumerate(q3[cut:cut + pad]):
            b = read_len + i
            words[r * wpr + b // 32] |= np.uint64(int(c)) << np.uint64(2 * (b % 32))
    lo = read_len - k - w
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, None)
    assert (want[2] > 0).all()
    _check(ctx, s, read_len, count, k, queries, lo, None, want, off=15, woff=1, words=words)


# ---- 3. identities on the device -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", (32, 33, 64))
def test_identity_with_best2_over_whole_short_reads(ctx, read_len):
    import torch
    rng = np.random.default_rng(read_len)
    for k, nq, count in ((1, 3, 70), (9, 33, 65), (17, 5, 200), (32, 2, 33)):
        queries, s = _random(rng, read_len, count, k, nq)
        t, ptr = _ascii_dev(s, 7)
        tw, wptr = _words_dev(ro.pack_reads(s, read_len, count), 1)
        dq = _dev_queries(queries)
        o = [Out(count) for _ in range(4)]
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o[0].ptrs())
        ctx.reads_hdist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o[1].ptrs())
        ctx.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *o[2].ptrs())
        ctx.reads_hdist_best2_packed_async(wptr, read_len, count, k, dq, nq, *o[3].ptrs())
        ctx.sync()
        got = [x.read() for x in o]
        want = r2.reads_best2(s, read_len, count, k, queries)
        assert all(_same(g, want) for g in got), (k, nq, [_diff(g, want) for g in got])


def test_identity_with_best2_on_a_compact_copy_of_the_spans(ctx):
    import torch
    rng = np.random.default_rng(150)
    read_len, count, k, nq = 150, 300, 16, 20
    queries, s = _random(rng, read_len, count, k, nq)
    t, ptr = _ascii_dev(s, 0)
    dq = _dev_queries(queries)
    for pos_lo, pos_hi in ((0, 3), (131, None), (50, 98)):
        hi, span = ra.span_of(read_len, k, pos_lo, pos_hi)
        spans = t[:count * read_len].view(count, read_len)[:, pos_lo:pos_lo + span].contiguous()  # the device-side compact copy
        o1, o2 = Out(count), Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=pos_lo, pos_hi=pos_hi)
        ctx.reads_hdist_best2_async(spans, span, count, k, dq, nq, *o2.ptrs())
        ctx.sync()
        got, ref = o1.read(), list(o2.read())
        for i in (1, 4):
            ref[i] = np.where(ref[i] != NO, ref[i] + np.uint32(pos_lo), ref[i]).astype(np.uint32)
        assert _same(got, ref), _diff(got, ref)
        assert _same(got, ra.reads_anchored(s, read_len, count, k, queries, pos_lo, pos_hi))


# ---- 4. further cases ------------------------------------------------------------------------------------------------------------------------
def test_null_second_pointers_write_the_best_triple_only(ctx):
    import torch
    rng = np.random.default_rng(9)
    read_len, count, k, nq = 65, 99, 13, 40
    queries, s = _random(rng, read_len, count, k, nq)
    want = ra.reads_anchored(s, read_len, count, k, queries, 2, 7)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(ro.pack_reads(s, read_len, count), 1)
    dq = _dev_queries(queries)
    for fn, src in ((ctx.reads_hdist_anchored_async, ptr), (ctx.reads_hdist_anchored_packed_async, wptr)):
        o = Out(count)
        torch.cuda.synchronize()
        fn(src, read_len, count, k, dq, nq, *o.ptrs(1), pos_lo=2, pos_hi=7)
        ctx.sync()
        assert o.untouched(triples=(1,)) and _same(o.read()[:3], want[:3])


def test_argument_errors_leave_the_outputs_untouched(ctx):
    import torch
    import bitnuc_amd as bn
    s = ro.LUT[np.random.default_rng(2).integers(0, 4, size=15000)].astype(np.uint8)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(ro.pack_reads(s, 150, 100), 0)
    dq = _dev_queries(np.zeros(16, dtype=np.uint64))
    o = Out(100)
    six = o.ptrs()
    torch.cuda.synchronize()
    for fn, src in ((ctx.reads_hdist_anchored_async, ptr), (ctx.reads_hdist_anchored_packed_async, wptr)):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 150, 100, 33, dq, 65537, *six, pos_lo=0, pos_hi=100)  # k first
        assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
        with pytest.raises(bn.NucleotideError) as ei:
            fn(src, 150, 100, 12, dq, 65537, *six, pos_lo=0, pos_hi=100)  # then the query count, before the span
        assert ei.value.kind == "Unsupported"
        for pos_lo, pos_hi, span in ((0, 53, 65), (0, None, 150), (80, None, 70)):
            err = _raw_err(fn, src, 150, 100, 12, dq, 16, six, pos_lo, pos_hi)
            assert err == ("Unsupported", span)
        for bad in ((six[0], six[1], six[2], 0, six[4], six[5]), (six[0], six[1], six[2], six[3], 0, 0), (six[0], six[1], six[2], six[3] + 2, six[4], six[5]),
                    (six[0], 0, six[2], six[3], six[4], six[5])):
            with pytest.raises(bn.NucleotideError) as ei:
                fn(src, 150, 100, 12, dq, 16, *bad, pos_lo=0, pos_hi=3)
            assert ei.value.kind == "Unsupported"
        del ei
    ctx.sync()
    assert o.untouched()


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


def test_invalid_bytes_inside_and_outside_the_spans(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, read_len, count, nq, lo, hi = 17, 150, 400, 33, 129, None  # the spans: bytes 129 .. 149 of every read
    queries, s = _random(rng, read_len, count, k, nq)
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    dq = _dev_queries(queries)
    b = s.copy()
    b[0], b[128], b[150 * 7 + 5], b[150 * 399 + 128] = ord("N"), ord("n"), 0, 0xFF  # outside every span
    for off in (0, 3):
        t, ptr = _ascii_dev(b, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o.read(ctx), want)  # no error, correct results
    for bad_at, off in ((150 * 200 + 129, 0), (150 * 0 + 149, 9), (150 * 399 + 140, 5)):  # a span's first byte, read 0's last, the last read
        c = b.copy()
        c[bad_at] = ord("N")
        if bad_at + 150 * 3 < c.size:
            c[bad_at + 150 * 3] = ord("x")  # a later one
        t, ptr = _ascii_dev(c, off)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing is left for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean and correct
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_async(ptr2, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o.read(ctx), want)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries on 64 reads with two offsets, against the host form in slices of 256 merged by reads_best2_oracle.merge_top2"""
    from bitnuc_amd import api
    rng = np.random.default_rng(65537)
    k, read_len, count, nq = 12, 60, 64, 65536
    queries = ro.random_queries(rng, nq, k)
    s = ro.random_reads(rng, read_len, count, k, queries[60000:], plant=8)
    free = api.context_free()
    assert _same(free.reads_hdist_anchored(s, read_len, k, queries[:64], pos_lo=47, pos_hi=None), ra.reads_anchored(s, read_len, count, k, queries[:64], 47, None))
    full = r2.merge_top2([(i, free.reads_hdist_anchored(s, read_len, k, queries[i:i + 256], pos_lo=47, pos_hi=None)) for i in range(0, nq, 256)])
    assert (full[5] != 0xFF).all()
    _check(ctx, s, read_len, count, k, queries, 47, None, full, 1, 1)


def test_graph_replay_after_the_reads_and_the_queries_changed():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    read_len, count, k, nq, lo, hi = 151, 2000, 31, 33, 0, 3
    (q1, s1), (q2, s2) = _random(rng, read_len, count, k, nq), _random(rng, read_len, count, k, nq)
    want1, want2 = ra.reads_anchored(s1, read_len, count, k, q1, lo, hi), ra.reads_anchored(s2, read_len, count, k, q2, lo, hi)
    assert not np.array_equal(want1[0], want2[0]) and not np.array_equal(want1[3], want2[3])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = ro.pack_reads(s1, read_len, count)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        o1, o2 = Out(count), Out(count)
        c.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi)  # warm-up outside the capture: sizes the scratch
        c.reads_hdist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi)
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi)
                c.reads_hdist_anchored_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi)
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


def test_mixed_queue_with_one_sync(ctx, oracle):
    """the anchored calls (ASCII and packed in turn) between reads_hdist_best2, kmer_hdist_best and encode_fixed on one context, different (count,
    n_queries) between consecutive calls (scratch 10 is laid out anew by each), one sync at the end, every result checked afterwards"""
    import torch
    rng = np.random.default_rng(809)
    k, read_len = 21, 150
    dev = torch.device("cuda:0")
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (800, 3))):  # inputs and outputs first
        queries, s = _random(rng, read_len, count, k, nq, lower=False)
        wpr = (read_len + 31) // 32
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries), out=Out(count), two=Out(count),
                         wdev=_words_dev(ro.pack_reads(s, read_len, count), i & 1), bpos=torch.zeros(nq, dtype=torch.int64, device=dev),
                         bdist=torch.zeros(nq, dtype=torch.uint8, device=dev), words=torch.zeros(count * wpr, dtype=torch.int64, device=dev),
                         rng=((0, 3), (126, None), (60, 80))[i % 3]))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, s, ptr, dq, (lo, hi) = j["i"], j["count"], j["nq"], j["s"], j["ascii"][1], j["dq"], j["rng"]
        if i % 2 == 0:
            ctx.reads_hdist_anchored_async(ptr, read_len, count, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        else:
            ctx.reads_hdist_anchored_packed_async(j["wdev"][1], read_len, count, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi)
        if i % 3 == 0:
            ctx.reads_hdist_best2_async(ptr, read_len, count, k, dq, nq, *j["two"].ptrs())
        elif i % 3 == 1:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, j["bpos"], j["bdist"])
        else:
            ctx.encode_fixed_dev(ptr, read_len, read_len, count, j["words"])
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, count, nq, s, queries, (lo, hi) = j["i"], j["count"], j["nq"], j["s"], j["queries"], j["rng"]
        want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        if i % 3 == 0:
            assert _same(j["two"].read(), r2.reads_best2_by_scan(oracle, s, read_len, count, k, queries)), i
        elif i % 3 == 1:
            scans = [oracle.kmer_hdist_scan(s, k, int(q)) for q in queries]
            assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i
        else:
            assert np.array_equal(j["words"].cpu().numpy().view(np.uint64), ro.pack_reads(s, read_len, count, junk=False)), i


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """900,000 reads of 150 bases, four offsets at the 3' end, three queries (10.8 * 10^6 offset-query pairs, above the default cutoff of 2^20) on a
    context with the default dispatch: the ASCII form's chunks are 894,784 whole reads (128 Mi bytes / 150), the packed form's 838,860 (4 Mi words / 5);
    the reads on both sides of each boundary hold a planted winner.  100,000 reads run in one chunk, 20,000 stay on the host.
    Then an N past the boundary, inside a span, reports its absolute index; one outside the spans is ignored."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    read_len, count, k, w = 150, 900_000, 25, 3
    lo = read_len - k - w
    per_ascii, per_packed = (128 << 20) // read_len, ((128 << 20) // 32) // 5
    assert per_packed < per_ascii < count
    queries = ro.random_queries(rng, 3, k)
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    near = [q.copy() for q in qc]
    for q in near:
        q[11] ^= 1
    for per in (per_ascii, per_packed):
        codes[per - 1, lo + 3:] = qc[0]   # the chunk's last read: query 0 at the last offset
        codes[per, lo:lo + k] = qc[1]     # the next chunk's first read: query 1 at the first offset
        codes[per + 1, lo + 1:lo + 1 + k] = near[2]
    s = ro.LUT[codes.reshape(-1)]
    del codes
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, None)
    for per in (per_ascii, per_packed):
        assert [_row(want, r)[:3] for r in (per - 1, per, per + 1)] == [(0, lo + 3, 0), (1, lo, 0), (2, lo + 1, 1)]
    c = bn.Context(0)
    try:
        got = c.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo)
        assert _same(got, want), _diff(got, want)
        words = c.encode_fixed(s, read_len).reshape(-1)
        got = c.reads_hdist_anchored_packed(words, read_len, count, k, queries, pos_lo=lo)
        assert _same(got, want), _diff(got, want)
        m, big = 20_000, 100_000  # 240,000 pairs: the host; 1.2 * 10^6 pairs: one chunk through the device
        assert m * 4 * 3 < 1 << 20 <= big * 4 * 3
        assert _same(c.reads_hdist_anchored(s[:big * read_len], read_len, k, queries, pos_lo=lo), tuple(a[:big] for a in want))
        assert _same(c.reads_hdist_anchored_packed(words[:big * 5], read_len, big, k, queries, pos_lo=lo, second=False), tuple(a[:big] for a in want[:3]))
        assert _same(c.reads_hdist_anchored(s[:m * read_len], read_len, k, queries, pos_lo=lo), tuple(a[:m] for a in want))  # stays on the host
        s[per_ascii * read_len + 7] = ord("N")  # outside the spans: ignored
        assert _same(c.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo), want)
        bad_at = per_ascii * read_len + lo + 9
        s[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
    finally:
        c.close()


def test_seeded_differential_fuzz(ctx):
    rng = np.random.default_rng(0xA2C4)
    for it in range(150):
        k = int(rng.integers(1, 33))
        offsets = int(rng.integers(1, 64 - k + 2)) if it % 3 else int(rng.choice((1, 2, 4)))
        read_len = int(rng.integers(offsets + k - 1, 201))
        count = int(rng.integers(1, (700, 130, 40, 300)[it % 4]))
        nq = int(rng.integers(1, 41))
        last = read_len - k
        kind = it % 4
        pos_lo = 0 if kind == 0 else (last + 1 - offsets if kind == 1 else int(rng.integers(0, last + 2 - offsets)))
        pos_hi = None if kind == 1 else pos_lo + offsets - 1
        queries, s = _random(rng, read_len, count, k, nq)
        _check(ctx, s, read_len, count, k, queries, pos_lo, pos_hi, off=int(rng.integers(0, 16)), woff=int(rng.integers(0, 2)),
               tag=(it, k, read_len, count, nq, pos_lo, pos_hi))
