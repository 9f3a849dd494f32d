"""GPU tests of the anchored best match and runner-up per read of a RAGGED batch (bitnuc_reads_hdist_anchored_batch[_packed]_async and the host forms
above the cutoff; reads_anchored_kernel under its ragged layout policy) against tests/reads_anchored_batch_oracle.py.  The tile is 32 reads x 32 (query,
offset) rows, a wave takes 64 reads at a time, K-steps end at 16 bases, and every read has its own first span base and its own number of admissible
offsets: counts around 32 / 64 and beyond the bounded grid, (queries, offsets) with rows per query of 1 .. 64 and queries astride tiles, k and spans
around the K-steps, lengths drawn so that the 32 reads of a tile all have different numbers of admissible offsets (0 included); both anchors throughout.
Planted cases: the overhang trap at k = 31 / 32 (a perfect copy of a query that starts 1 .. 3 bases too late in a read, completed by the next read's
first bases, by the packed pad bits, or by the bytes behind the batch), matches at the first and the last admissible offset with better ones just
outside, ties, duplicates and the winner's second window.  Invalid bytes inside and outside the spans; NULL second pointers; argument errors; the
query limit; a hipGraph replay after the lengths changed; a queue of mixed calls; the host forms in one chunk and across two; the identities with the
fixed anchored form and with reads_hdist_best_batch on the device; a seeded differential fuzz.  Both _async forms run on the same data: ASCII at byte
offsets +0 / +1 / +7 / +15 with lowercase bases, packed words at 16-byte and 8-mod-16 offsets with junk pad bits.  Every comparison is exact equality of
all written arrays; guard words and bytes surround all six outputs and both dist arrays start at odd byte offsets."""
import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_batch_oracle as rb
import reads_anchored_batch_oracle as rab

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
NO = ro.NO_U32
OFFS = (0, 1, 7, 15)
START, END = 0, 1
BOTH = (START, END)


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


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


def _ascii_dev(s, off, behind=None):
    """s at byte offset `off` of a device buffer; `behind`: the bytes right behind the batch (default zeros: invalid, must never be examined)"""
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    if behind is not None:
        t[off + s.size:off + s.size + len(behind)] = torch.from_numpy(np.asarray(behind, dtype=np.uint8))
    return t, t.data_ptr() + off


def _words_dev(w, off, behind=None):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    if behind is not None:
        t[off + w.size:off + w.size + len(behind)] = torch.from_numpy(np.asarray(behind, dtype=np.uint64).view(np.int64))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero(np.any([g != w for g, w in zip(got, want)], axis=0))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


def _row(want, r):
    return tuple(int(a[r]) for a in want)


def _both(ctx, s, off, k, queries, anchor, lo, hi, aoff=0, woff=0, words=None, behind=None, wbehind=None):
    """(six arrays of the ASCII form, six of the packed form), guards checked"""
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count, nq = off.size - 1, len(queries)
    wtab = rb.word_offsets_of(off)
    w = rb.pack_batch(s, off, seed=k) if words is None else words
    t, ptr = _ascii_dev(s, aoff, behind)
    tw, wptr = _words_dev(w, woff, wbehind)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_u64(queries)
    o1, o2 = Out(count), Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
    ctx.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check(ctx, s, off, k, queries, anchor, lo, hi, want=None, aoff=0, woff=0, words=None, behind=None, wbehind=None, tag=()):
    if want is None:
        want = rab.reads_anchored_batch(s, off, k, queries, anchor, lo, hi)
    a, p = _both(ctx, s, off, k, queries, anchor, lo, hi, aoff, woff, words, behind, wbehind)
    assert _same(a, want), ("ascii", tag, _diff(a, want))
    assert _same(p, want), ("packed", tag, _diff(p, want))
    return want


def _tile_lengths(rng, count, k, lo, width):
    """lengths in tiles of 32 consecutive reads that all have different numbers of admissible offsets where the range is wide enough (n = min(len - k - lo,
    width - 1) + 1 for either anchor: 0 at k + lo - 1 bases, width from k + lo + width - 1 on), with empty reads, reads of 1 .. k - 1 bases and much
    longer ones mixed in"""
    base = k + lo - 1
    out = []
    while len(out) < count:
        tile = [base + j for j in range(min(32, width + 1))]
        while len(tile) < 32:
            tile.append(int(rng.choice((0, max(k - 1, 0), k, base + width, base + width + 1, base + width + int(rng.integers(2, 200))))))
        rng.shuffle(tile)
        out += tile
    return out[:count]


def _random(rng, lengths, k, nq):
    queries = ro.random_queries(rng, nq, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    return queries, s, off


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 31, 32, 33, 63, 64, 65, 129))
def test_counts_around_the_tile_and_the_wave(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, nq, lo, width) in enumerate(((16, 17, 0, 4), (31, 3, 2, 11), (5, 33, 0, 1))):
        queries, s, off = _random(rng, _tile_lengths(rng, count, k, lo, width), k, nq)
        for anchor in BOTH:
            _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[(i + count) % 4], woff=(i + count) % 2, tag=(count, k, lo, width, anchor))


def test_a_count_beyond_the_bounded_grid(ctx):
    """more blocks of 64 reads than the grid has waves (at most 4 workgroups of four waves per CU): some waves loop; reads of 20 .. 40 bases"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 256 + 8263
    rng = np.random.default_rng(5)
    k, nq = 12, 5
    queries, s, off = _random(rng, rng.integers(20, 41, size=count), k, nq)
    _check(ctx, s, off, k, queries, END, 0, 3, aoff=1, woff=1)
    _check(ctx, s, off, k, queries, START, 14, 17, aoff=7, woff=0)


@pytest.mark.parametrize("nq,width,k", ((1, 1, 16), (1, 33, 32), (3, 1, 16), (33, 1, 16), (3, 2, 15), (17, 2, 31), (17, 4, 16), (33, 4, 16), (3, 8, 17), (17, 8, 9),
                                        (1, 16, 9), (33, 16, 32), (3, 32, 22), (17, 32, 2), (3, 64, 1), (17, 40, 2), (33, 11, 21)))
def test_queries_and_offsets_around_the_tile(ctx, nq, width, k):
    """rows per query of 1, 2, 4, 8, 16 (several queries per lane), 32 (a query per tile) and 64 (a query per two tiles), queries astride tiles; 40 and 11
    offsets: rows that no read admits; the last tile partly empty"""
    rng = np.random.default_rng(1000 * nq + width)
    for lo in (0, 3):
        queries, s, off = _random(rng, _tile_lengths(rng, 70, k, lo, width), k, nq)
        for anchor in BOTH:
            _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[(nq + width) % 4], woff=nq % 2, tag=(nq, width, k, lo, anchor))


@pytest.mark.parametrize("k", (1, 2, 15, 16, 17, 21, 22, 31, 32))
def test_k_and_spans_around_the_k_steps(ctx, k):
    rng = np.random.default_rng(40 + k)
    for span in sorted({k, 16, 17, 21, 22, 32, 33, 48, 49, 64}):
        if span < k:
            continue
        width = span - k + 1
        lo = (0, 1, 30)[span % 3]
        nq = (1, 2, 5, 33)[(span + k) % 4]
        queries, s, off = _random(rng, _tile_lengths(rng, 67, k, lo, width), k, nq)
        for anchor in BOTH:
            _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[(span + k) % 4], woff=span % 2, tag=(k, span, lo, anchor))


@pytest.mark.parametrize("k,width", ((16, 32), (31, 34), (32, 33), (8, 57), (1, 64)))
def test_the_32_reads_of_a_tile_all_have_different_numbers_of_admissible_offsets(ctx, k, width):
    rng = np.random.default_rng(320 + k)
    for lo in (0, 4):
        lengths = _tile_lengths(rng, 96, k, lo, width)
        for anchor in BOTH:
            first, n = rab.windows(lengths, k, anchor, lo, lo + width - 1)
            for t in range(3):
                assert len(set(n[32 * t:32 * t + 32].tolist())) == 32 and 0 in n[32 * t:32 * t + 32]
        queries, s, off = _random(rng, lengths, k, 6)
        for anchor in BOTH:
            want = _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=15, woff=1, tag=(k, width, lo, anchor))
            assert ((want[2] == 0xFF) == (n == 0)).all()


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (31, 32))
def test_the_overhang_trap(ctx, k):
    """Range 0 .. 4 (START: offsets 0 .. 4; END: the last k bases with four bases of slack).  A read of k + 1 bases admits offsets 0 and 1; a perfect copy
    of query 1 starts at offset 2, 3 or 4 of it -- 1, 2 or 3 bases too late -- and the next read's first bases (ASCII), the read's pad bits (packed)
    or, for the last read, the bytes and the word behind the batch complete it: the rows of those offsets are live in the tile (the longer neighbours
    admit them) and would reach distance 0.  It must not be reported.  Reads of k - 1, k - 2 and k - 3 bases that are a prefix of the query, completed
    the same way, have no admissible window: the fill."""
    rng = np.random.default_rng(3100 + k)
    nq = 3
    queries = ro.random_queries(rng, nq, k)
    q1 = ro.query_codes(queries[1], k)
    lengths, plan = [], []
    for r in range(70):
        kind = r % 7
        if kind < 3:    # a copy that starts kind + 1 bases too late in a read of k + 1 bases
            lengths.append(k + 1), plan.append((2 + kind, k + 1 - (2 + kind)))
        elif kind < 6:  # a prefix of the query, kind - 2 bases short: no window
            lengths.append(k - (kind - 2)), plan.append((0, k - (kind - 2)))
        else:           # a long read: every offset admissible
            lengths.append(k + 20), plan.append(None)
    lengths[-1], plan[-1] = k + 1, (3, k - 2)  # the last read: completed by what lies behind the batch
    lengths[-2], plan[-2] = k - 1, (0, k - 1)
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    pads = {}
    for r, p in enumerate(plan):
        if p is None:
            continue
        at, have = p
        o = int(off[r])
        codes[o + at:o + at + have] = q1[:have]
        rest = q1[have:]
        nxt = int(off[r + 1])
        m = min(len(rest), codes.size - nxt)
        codes[nxt:nxt + m] = rest[:m]  # the next read's first bases (the read after it may overwrite some: the trap then closes on fewer reads)
        pads[r] = list(rest)
    for r, p in enumerate(plan):  # re-plant the reads' own parts: a later neighbour's completion must not have damaged them
        if p is not None:
            o = int(off[r])
            codes[o + p[0]:o + p[0] + p[1]] = q1[:p[1]]
    s = ro.LUT[codes].astype(np.uint8)
    s[::5] |= 0x20
    last_rest = q1[plan[-1][1]:]
    behind = ro.LUT[np.asarray(last_rest)].astype(np.uint8)
    words = rb.pack_batch(s, off, pad_codes=pads)
    wbehind = np.array([ro.word_of([3] * 32)], dtype=np.uint64)
    trapped = [r for r, p in enumerate(plan) if p is not None and lengths[r] == k + 1]
    short = [r for r, p in enumerate(plan) if p is not None and lengths[r] < k]
    closed = 0
    for r in trapped[:-1]:  # the ASCII trap is closed where the bytes behind the read really spell the rest of the query
        o, (at, have) = int(off[r]), plan[r]
        closed += bool(np.array_equal(codes[o + at:o + at + k], q1))
    assert closed >= 10
    for anchor in BOTH:
        want = rab.reads_anchored_batch(s, off, k, queries, anchor, 0, 4)
        assert all(int(want[2][r]) > 0 and int(want[2][r]) != 0xFF for r in trapped), "the oracle sees no match in a trapped read"
        assert all(_row(want, r) == (NO, NO, 0xFF, NO, NO, 0xFF) for r in short)
        for aoff, woff in ((0, 0), (1, 1), (7, 0), (15, 1)):
            _check(ctx, s, off, k, queries, anchor, 0, 4, want, aoff, woff, words=words, behind=behind, wbehind=wbehind, tag=(k, anchor, aoff))


def _planted(rng, k=20, nq=24):
    """END (2, 12) on reads of 90, 61, 75, 50, 66, 20 and 19 bases (and 64 random ones): query 3 and its equal duplicate 20 exactly in read 0; an exact
    copy of query 5 one base in front of read 1's range and one base behind read 2's; query 12 at the last admissible offset of read 3 and the first of
    read 4; read 5's last offset is below pos_lo, read 6 is shorter than k"""
    queries = ro.random_queries(rng, nq, k)
    queries[20] = queries[3] ^ (np.uint64(1) << np.uint64(63))
    lengths = [90, 61, 75, 50, 66, 20, 19] + list(rng.integers(0, 120, size=64))
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    q3, q5, q12 = (ro.query_codes(queries[i], k) for i in (3, 5, 12))
    near5 = q5.copy()
    near5[[2, 9]] ^= 1
    o = [int(x) for x in off]
    codes[o[0] + 60:o[0] + 60 + k] = q3
    codes[o[1] + 28:o[1] + 28 + k], codes[o[1] + 5:o[1] + 5 + k] = q5, near5
    codes[o[2] + 54:o[2] + 54 + k], codes[o[2] + 20:o[2] + 20 + k] = q5, near5
    codes[o[3] + 28:o[3] + 28 + k] = q12
    codes[o[4] + 34:o[4] + 34 + k] = q12
    s = ro.LUT[codes].astype(np.uint8)
    s[::3] |= 0x20
    return queries, s, off


def test_first_and_last_admissible_offsets_better_matches_outside_and_duplicates(ctx):
    rng = np.random.default_rng(35)
    k = 20
    queries, s, off = _planted(rng, k)
    want = rab.reads_anchored_batch(s, off, k, queries, END, 2, 12)
    assert _row(want, 0) == (3, 60, 0, 20, 60, 0) and _row(want, 3)[:3] == (12, 28, 0) and _row(want, 4)[:3] == (12, 34, 0)
    assert int(want[2][1]) > 0 and int(want[2][2]) > 0 and int(want[3][3]) != 12 and int(want[3][4]) != 12
    assert _row(want, 5) == (NO, NO, 0xFF, NO, NO, 0xFF) and _row(want, 6) == (NO, NO, 0xFF, NO, NO, 0xFF)
    for aoff, woff in ((0, 0), (7, 1)):
        _check(ctx, s, off, k, queries, END, 2, 12, want, aoff, woff)
    # START (29, 39) puts the same questions to read 1 (the copy at 28 is one base in front) and START (43, 53) to read 2 (54: one base behind)
    for lo, hi, r in ((29, 39, 1), (43, 53, 2)):
        want = _check(ctx, s, off, k, queries, START, lo, hi, aoff=1, woff=1)
        assert int(want[2][r]) > 0
    want = _check(ctx, s, off, k, queries, START, 28, 54, aoff=15)  # one offset wider on either side: both copies are found
    assert _row(want, 1)[:3] == (5, 28, 0) and _row(want, 2)[:3] == (5, 54, 0)


@pytest.mark.parametrize("orig,dup,nq", ((4, 5, 24), (1, 6, 24), (4, 9, 24), (4, 300, 304)))
def test_ties_duplicates_and_the_winners_second_window(ctx, orig, dup, nq):
    """Four offsets: a tile holds eight queries, 0 .. 3 in the registers of lane l, 4 .. 7 in those of lane l ^ 32.  An equal duplicate query (the same
    lane, the partner lane, the next tile, a far tile) is the runner-up at the same offset; the winner at a second admissible offset (distance 1) is
    not; poly-A reads and a poly-A query: the lowest admissible offset of each read"""
    rng = np.random.default_rng(600 + dup)
    k, lo, hi = 16, 1, 4
    lengths = [int(x) for x in rng.integers(k + 6, 70, size=37)] + [k + 2, k + 1, k]
    queries = ro.random_queries(rng, nq, k)
    queries[dup] = queries[orig] ^ (np.uint64(1) << np.uint64(63))
    qo = ro.query_codes(queries[orig], k)
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    for r, ln in enumerate(lengths[:37]):  # END (1, 4): offsets last - 4 .. last - 1; the query at last - 2, and with one change 16 bases in front
        o, last = int(off[r]), ln - k
        codes[o + last - 2:o + ln - 2] = qo
    s = ro.LUT[codes].astype(np.uint8)
    want = rab.reads_anchored_batch(s, off, k, queries, END, lo, hi)
    for r, ln in enumerate(lengths[:37]):
        assert _row(want, r) == (orig, ln - k - 2, 0, dup, ln - k - 2, 0)
    assert _row(want, 39) == (NO, NO, 0xFF, NO, NO, 0xFF) and int(want[1][38]) == 0 and int(want[2][38]) != 0xFF  # k bases: no window; k + 1: offset 0
    _check(ctx, s, off, k, queries, END, lo, hi, want, aoff=1, woff=0)
    queries[0] = 0
    s = np.full(int(off[-1]), ord("A"), dtype=np.uint8)
    for anchor in BOTH:
        want = _check(ctx, s, off, k, queries, anchor, lo, hi, aoff=15, woff=1)
        first, n = rab.windows(lengths, k, anchor, lo, hi)
        assert np.array_equal(want[1][n > 0], first[n > 0].astype(np.uint32)) and (want[0][n > 0] == 0).all() and (want[2][n > 0] == 0).all()


# ---- 3. identities on the device -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_", (33, 64, 150))
def test_identity_with_the_fixed_anchored_form_on_equal_lengths(ctx, L_):
    import torch
    rng = np.random.default_rng(L_)
    count = 131
    for k, nq in ((1, 3), (16, 17), (32, 5)):
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, L_, count, k, queries)
        off = rb.offsets_of([L_] * count)
        wtab = rb.word_offsets_of(off)
        words = ro.pack_reads(s, L_, count)
        t, ptr = _ascii_dev(s, 7)
        tw, wptr = _words_dev(words, 1)
        d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_u64(queries)
        last = L_ - k
        for e_lo, e_hi in ((0, 0), (0, min(3, last)), (min(2, last), min(9, last))):
            o = [Out(count) for _ in range(6)]
            torch.cuda.synchronize()
            lo, hi = last - e_hi, last - e_lo
            ctx.reads_hdist_anchored_async(ptr, L_, count, k, dq, nq, *o[0].ptrs(), pos_lo=lo, pos_hi=hi)
            ctx.reads_hdist_anchored_packed_async(wptr, L_, count, k, dq, nq, *o[1].ptrs(), pos_lo=lo, pos_hi=hi)
            ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o[2].ptrs(), pos_lo=e_lo, pos_hi=e_hi, anchor="end")
            ctx.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o[3].ptrs(), pos_lo=e_lo, pos_hi=e_hi, anchor="end")
            ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o[4].ptrs(), pos_lo=lo, pos_hi=hi, anchor="start")
            ctx.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o[5].ptrs(), pos_lo=lo, pos_hi=hi, anchor="start")
            ctx.sync()
            got = [x.read() for x in o]
            assert all(_same(g, got[0]) for g in got[1:]), (k, e_lo, e_hi, [_diff(g, got[0]) for g in got[1:]])
            assert _same(got[0], rab.reads_anchored_batch(s, off, k, queries, END, e_lo, e_hi))


def test_identity_with_best_batch_on_reads_of_at_most_64_bases(ctx):
    import torch
    rng = np.random.default_rng(64)
    for k, nq in ((1, 3), (16, 9), (31, 17), (32, 2)):
        lengths = list(rng.integers(0, 65, size=200)) + [0, k - 1, k, 64]
        count = len(lengths)
        queries, s, off = _random(rng, lengths, k, nq)
        wtab = rb.word_offsets_of(off)
        t, ptr = _ascii_dev(s, 1)
        tw, wptr = _words_dev(rb.pack_batch(s, off), 1)
        d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_u64(queries)
        o = [Out(count), Out(count), Out(count, 1), Out(count, 1)]
        torch.cuda.synchronize()
        ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o[0].ptrs(), pos_lo=0, pos_hi=64 - k, anchor="start")
        ctx.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o[1].ptrs(), pos_lo=0, pos_hi=64 - k, anchor="start")
        ctx.reads_hdist_best_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o[2].ptrs())
        ctx.reads_hdist_best_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o[3].ptrs())
        ctx.sync()
        got = [x.read() for x in o]
        want = rb.batch_best(s, off, k, queries)
        assert all(_same(g[:3], want) for g in got), (k, nq)


# ---- 4. further cases ------------------------------------------------------------------------------------------------------------------------
def test_null_second_pointers_write_the_best_triple_only(ctx):
    import torch
    rng = np.random.default_rng(9)
    k, nq = 13, 40
    queries, s, off = _random(rng, _tile_lengths(rng, 99, k, 0, 6), k, nq)
    count = off.size - 1
    wtab = rb.word_offsets_of(off)
    want = rab.reads_anchored_batch(s, off, k, queries, END, 0, 5)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 1)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_u64(queries)
    for packed in (False, True):
        o = Out(count)
        torch.cuda.synchronize()
        if packed:
            ctx.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o.ptrs(1), pos_lo=0, pos_hi=5, anchor="end")
        else:
            ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(1), pos_lo=0, pos_hi=5, anchor="end")
        ctx.sync()
        assert o.untouched(triples=(1,)) and _same(o.read()[:3], want[:3])


def _raw_err(ctx, packed, head, k, anchor, lo, hi, dq, nq, six):
    """(status, value) of a device call through the raw entry point (the Python error carries no value for Unsupported)"""
    import ctypes as C
    from bitnuc_amd import _lib as L
    raw = L.load().bitnuc_reads_hdist_anchored_batch_packed_async if packed else L.load().bitnuc_reads_hdist_anchored_batch_async
    err = L.BitnucErr()
    st = raw(ctx._h, *(C.c_void_p(p) if i < (3 if packed else 2) else p for i, p in enumerate(head)), k, anchor, lo, hi, C.c_void_p(dq.data_ptr()), nq,
             *(C.c_void_p(p) if p else None for p in six), C.byref(err))
    return st, int(err.value)


def test_argument_errors_leave_the_outputs_untouched(ctx):
    import torch
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(2)
    k = 12
    queries, s, off = _random(rng, rng.integers(0, 150, size=100), k, 16)
    count, total = 100, int(off[-1])
    wtab = rb.word_offsets_of(off)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 0)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_u64(queries)
    o = Out(count)
    six = o.ptrs()
    size_max = 2**64 - 1
    torch.cuda.synchronize()
    for packed, head in ((False, (ptr, d_off.data_ptr(), count, total)), (True, (wptr, d_wtab.data_ptr(), d_off.data_ptr(), count, int(wtab[-1])))):
        assert _raw_err(ctx, packed, head, 33, 7, 0, size_max, dq, 65537, six) == (L.SEQUENCE_TOO_LONG, 33)  # k first
        big = head[:-1] + (2**58 if not packed else 2**53,)
        assert _raw_err(ctx, packed, big, k, 7, 0, size_max, dq, 65537, six) == (L.UNSUPPORTED, big[-1])     # then the totals' limit
        assert _raw_err(ctx, packed, head, k, 7, 0, size_max, dq, 65537, six) == (L.UNSUPPORTED, 65537)      # the query count
        assert _raw_err(ctx, packed, head, k, 2, 0, size_max, dq, 16, six) == (L.UNSUPPORTED, 2)             # the anchor
        assert _raw_err(ctx, packed, head, k, END, 0, size_max, dq, 16, six) == (L.UNSUPPORTED, size_max)    # the span
        assert _raw_err(ctx, packed, head, k, END, 0, 53, dq, 16, six) == (L.UNSUPPORTED, 65)
        for bad in ((six[0], six[1], six[2], 0, six[4], six[5]), (six[0], six[1], six[2], six[3], 0, 0), (six[0], six[1], six[2], six[3] + 2, six[4], six[5]),
                    (six[0], 0, six[2], six[3], six[4], six[5])):
            assert _raw_err(ctx, packed, head, k, END, 0, 3, dq, 16, bad) == (L.UNSUPPORTED, 0)
        tabs = (1,) if not packed else (1, 2)
        for i in tabs:  # a table NULL or not 8-byte aligned
            for v in (0, head[i] + 4):
                assert _raw_err(ctx, packed, head[:i] + (v,) + head[i + 1:], k, END, 0, 3, dq, 16, six) == (L.UNSUPPORTED, 0)
        assert _raw_err(ctx, packed, (0,) + head[1:], k, END, 0, 3, dq, 16, six) == (L.UNSUPPORTED, 0)      # the data, last
        if packed:
            assert _raw_err(ctx, packed, (wptr + 4,) + head[1:], k, END, 0, 3, dq, 16, six) == (L.UNSUPPORTED, 0)
    ctx.sync()
    assert o.untouched()
    # no window from the host-known arguments: the fill, even with NULL data (the packed form knows the words' total only: 32 bases per word)
    room = 32 * int(wtab[-1])
    for kk, nq, lo, hi in ((0, 16, 0, 3), (k, 0, 0, 3), (k, 16, 5, 4), (k, 16, room, room + 3)):
        for packed, head in ((False, (0, d_off.data_ptr(), count, total)), (True, (0, d_wtab.data_ptr(), d_off.data_ptr(), count, int(wtab[-1])))):
            o = Out(count)
            torch.cuda.synchronize()
            assert _raw_err(ctx, packed, head, kk, START, lo, hi, dq, nq, o.ptrs()) == (L.OK, 0)
            assert _same(o.read(ctx), r2.fill6(count)), (kk, nq, lo, hi)
    o = Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_anchored_batch_async(ptr, d_off, 0, total, k, dq, 16, *o.ptrs(), pos_lo=0, pos_hi=3)  # count == 0: nothing written
    ctx.sync()
    assert o.untouched()


def test_invalid_bytes_inside_and_outside_the_spans(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, nq, lo, hi = 17, 33, 2, 5
    lengths = _tile_lengths(rng, 400, k, lo, 4)
    queries, s, off = _random(rng, lengths, k, nq)
    count = off.size - 1
    dq, d_off = _dev_u64(queries), _dev_u64(off)
    for anchor in BOTH:
        want = rab.reads_anchored_batch(s, off, k, queries, anchor, lo, hi)
        mask = rab.span_bytes(off, k, anchor, lo, hi)
        b = s.copy()
        b[~mask] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=int((~mask).sum()))  # every byte that no span holds is invalid
        for aoff in (0, 3):
            t, ptr = _ascii_dev(b, aoff)
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert _same(o.read(ctx), want)  # no error, correct results
        spans = np.nonzero(mask)[0]
        for bad_at, aoff in ((int(spans[spans.size // 2]), 0), (int(spans[0]), 9), (int(spans[-1]), 5)):
            c = b.copy()
            c[bad_at] = ord("N")
            later = spans[spans > bad_at + 300]
            if later.size:
                c[int(later[0])] = ord("x")  # a later one
            t, ptr = _ascii_dev(c, aoff)
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
            del ei
            ctx.sync()  # latched once: nothing is left for the next sync
            t2, ptr2 = _ascii_dev(b, aoff)  # the next call on the same context is clean and correct
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_hdist_anchored_batch_async(ptr2, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert _same(o.read(ctx), want)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries on 64 ragged reads with two offsets at the end, against the host form in slices of 256 merged by
    reads_best2_oracle.merge_top2 (the host form itself is held against the oracle on the first slice)"""
    from bitnuc_amd import api
    rng = np.random.default_rng(65537)
    k, nq = 12, 65536
    lengths = [int(x) for x in rng.integers(11, 60, size=64)]
    queries = ro.random_queries(rng, nq, k)
    s, off = rb.random_batch(rng, lengths, k, queries[60000:])
    free = api.context_free()
    assert _same(free.reads_hdist_anchored_batch(s, off, k, queries[:64], pos_lo=0, pos_hi=1, anchor="end"), rab.reads_anchored_batch(s, off, k, queries[:64], END, 0, 1))
    full = r2.merge_top2([(i, free.reads_hdist_anchored_batch(s, off, k, queries[i:i + 256], pos_lo=0, pos_hi=1, anchor="end")) for i in range(0, nq, 256)])
    _check(ctx, s, off, k, queries, END, 0, 1, full, 1, 1)


def test_graph_replay_after_the_lengths_changed():
    """the tables are read on the device at every replay: the same count and totals, other lengths (and other reads and queries) give the new answers"""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    k, nq, lo, hi, count = 31, 33, 0, 3, 2000
    l1 = np.array(_tile_lengths(rng, count, k, lo, 4))
    l1[l1 % 32 == 0] += 1  # no multiple of 32: a permutation then keeps the words' total as well
    l2 = rng.permutation(l1)
    (q1, s1, off1), (q2, s2, off2) = _random(rng, l1, k, nq), _random(rng, l2, k, nq)
    w1tab, w2tab = rb.word_offsets_of(off1), rb.word_offsets_of(off2)
    assert int(off1[-1]) == int(off2[-1]) and int(w1tab[-1]) == int(w2tab[-1]) and not np.array_equal(off1, off2)
    want1, want2 = rab.reads_anchored_batch(s1, off1, k, q1, END, lo, hi), rab.reads_anchored_batch(s2, off2, k, q2, END, lo, hi)
    assert not np.array_equal(want1[1], want2[1])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = rb.pack_batch(s1, off1)
        tw, wptr = _words_dev(w, 1)
        dq, d_off, d_wtab = _dev_u64(q1), _dev_u64(off1), _dev_u64(w1tab)
        o1, o2 = Out(count), Out(count)

        def run():
            c.reads_hdist_anchored_batch_async(ptr, d_off, count, int(off1[-1]), k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi, anchor="end")
            c.reads_hdist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(w1tab[-1]), k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi, anchor="end")
        run()  # warm-up outside the capture: sizes the scratch
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                run()
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(rb.pack_batch(s2, off2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_u64(q2))
            d_off.copy_(_dev_u64(off2))
            d_wtab.copy_(_dev_u64(w2tab))
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
    """the ragged anchored calls (ASCII and packed in turn, both anchors) between the fixed anchored form, reads_hdist_best_batch and kmer_hdist_best on
    one context, different (count, n_queries) between consecutive calls (scratch 10 is laid out anew by each), one sync at the end"""
    import torch
    rng = np.random.default_rng(809)
    k = 21
    dev = torch.device("cuda:0")
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (800, 3))):  # inputs and outputs first
        lengths = rng.integers(0, 90, size=count) if i % 3 else np.full(count, 64)
        queries, s, off = _random(rng, lengths, k, nq)
        wtab = rb.word_offsets_of(off)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, off=off, wtab=wtab, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_u64(queries),
                         d_off=_dev_u64(off), d_wtab=_dev_u64(wtab), out=Out(count), two=Out(count), one=Out(count, 1), wdev=_words_dev(rb.pack_batch(s, off), i & 1),
                         bpos=torch.zeros(nq, dtype=torch.int64, device=dev), bdist=torch.zeros(nq, dtype=torch.uint8, device=dev),
                         anchor=("end", "start")[(i >> 1) & 1], rng=((0, 3), (2, 2), (1, 20))[i % 3]))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, ptr, dq, (lo, hi) = j["i"], j["count"], j["nq"], j["ascii"][1], j["dq"], j["rng"]
        if i % 2 == 0:
            ctx.reads_hdist_anchored_batch_async(ptr, j["d_off"], count, int(j["off"][-1]), k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi, anchor=j["anchor"])
        else:
            ctx.reads_hdist_anchored_batch_packed_async(j["wdev"][1], j["d_wtab"], j["d_off"], count, int(j["wtab"][-1]), k, dq, nq, *j["out"].ptrs(), pos_lo=lo,
                                                        pos_hi=hi, anchor=j["anchor"])
        if i % 3 == 0:
            ctx.reads_hdist_anchored_async(ptr, 64, count, k, dq, nq, *j["two"].ptrs(), pos_lo=lo, pos_hi=hi)
        elif i % 3 == 1:
            ctx.reads_hdist_best_batch_async(ptr, j["d_off"], count, int(j["off"][-1]), k, dq, nq, *j["one"].ptrs())
        else:
            ctx.kmer_hdist_best_async(ptr, j["s"].size, k, dq, nq, j["bpos"], j["bdist"])
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, nq, s, off, queries, (lo, hi) = j["i"], j["nq"], j["s"], j["off"], j["queries"], j["rng"]
        anchor = END if j["anchor"] == "end" else START
        want = rab.reads_anchored_batch(s, off, k, queries, anchor, lo, hi)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        if i % 3 == 0:
            assert _same(j["two"].read(), rab.reads_anchored_batch(s, off, k, queries, START, lo, hi)), i
        elif i % 3 == 1:
            assert _same(j["one"].read(), rb.batch_best(s, off, k, queries)), i
        else:
            scans = [rb.numpy_scan(s, k, int(q)) for q in queries]
            assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """1,150,000 reads of 100 .. 140 bases, END (0, 3), three queries (13.8 * 10^6 offset-query pairs, above the default cutoff of 2^20) on a context with
    the default dispatch: the ASCII form's first chunk is the longest run of whole reads within 128 Mi bytes, the packed form's within 4 Mi words; the
    reads on both sides of each boundary hold a planted winner.  100,000 reads run in one chunk, 20,000 stay on the host.  Then an N past the
    boundary, inside a span, reports its absolute index; one outside the spans is ignored."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    count, k = 1_150_000, 25
    lengths = rng.integers(100, 141, size=count)
    off = rb.offsets_of(lengths)
    wtab = rb.word_offsets_of(off)
    per_ascii = int(np.searchsorted(off, 128 << 20, side="right")) - 1    # the first chunk's reads: the largest r1 with off[r1] <= the budget
    per_packed = int(np.searchsorted(wtab, (128 << 20) // 32, side="right")) - 1
    assert 0 < per_packed < per_ascii < count
    queries = ro.random_queries(rng, 3, k)
    codes = rng.integers(0, 4, size=int(off[-1]), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    near = qc[2].copy()
    near[11] ^= 1
    o = off.astype(np.int64)
    for per in (per_ascii, per_packed):
        codes[o[per] - k:o[per]] = qc[0]                    # the chunk's last read: query 0 in its last k bases
        codes[o[per + 1] - k - 3:o[per + 1] - 3] = qc[1]    # the next chunk's first read: query 1 three bases in front of the end
        codes[o[per + 2] - k - 1:o[per + 2] - 1] = near
    s = ro.LUT[codes]
    del codes
    want = rab.reads_anchored_batch(s, off, k, queries, END, 0, 3)
    for per in (per_ascii, per_packed):
        ln = [int(lengths[r]) for r in (per - 1, per, per + 1)]
        assert [_row(want, r)[:3] for r in (per - 1, per, per + 1)] == [(0, ln[0] - k, 0), (1, ln[1] - k - 3, 0), (2, ln[2] - k - 1, 1)]
    c = bn.Context(0)
    try:
        got = c.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert _same(got, want), _diff(got, want)
        words = rb.pack_batch(s, off)
        got = c.reads_hdist_anchored_batch_packed(words, wtab, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert _same(got, want), _diff(got, want)
        m, big = 20_000, 100_000  # 240,000 pairs: the host; 1.2 * 10^6 pairs: one chunk through the device
        assert m * 4 * 3 < 1 << 20 <= big * 4 * 3
        assert _same(c.reads_hdist_anchored_batch(s, off[:big + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end"), tuple(a[:big] for a in want))
        assert _same(c.reads_hdist_anchored_batch_packed(words, wtab[:big + 1], off[:big + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end", second=False),
                     tuple(a[:big] for a in want[:3]))
        assert _same(c.reads_hdist_anchored_batch(s, off[:m + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end"), tuple(a[:m] for a in want))  # stays on the host
        s[int(o[per_ascii]) + 7] = ord("N")  # outside the spans: ignored
        assert _same(c.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=3, anchor="end"), want)
        bad_at = int(o[per_ascii + 1]) - 9
        s[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
    finally:
        c.close()


def test_seeded_differential_fuzz(ctx):
    rng = np.random.default_rng(0xA2C5)
    for it in range(40):
        k = int(rng.integers(1, 33))
        width = int(rng.integers(1, 64 - k + 2)) if it % 3 else int(rng.choice((1, 2, 4)))
        lo = int(rng.integers(0, 40)) if it % 2 else 0
        count = int(rng.integers(1, (700, 130, 40, 300)[it % 4]))
        nq = int(rng.integers(1, 41))
        kind = it % 4
        if kind == 0:
            lengths = _tile_lengths(rng, count, k, lo, width)
        elif kind == 1:
            lengths = rng.integers(0, 2 * (k + lo + width), size=count)
        elif kind == 2:
            lengths = rng.integers(max(0, k + lo - 2), k + lo + width + 2, size=count)
        else:
            lengths = rng.integers(0, 200, size=count)
        queries, s, off = _random(rng, lengths, k, nq)
        _check(ctx, s, off, k, queries, BOTH[(it >> 2) & 1], lo, lo + width - 1, aoff=int(rng.integers(0, 16)), woff=int(rng.integers(0, 2)),
               tag=(it, k, width, lo, count, nq))
