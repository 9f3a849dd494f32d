"""GPU tests of the per-read matchers under pattern queries (bitnuc_reads_pattern_best*, _best2*, _best_batch*, _anchored*, _anchored_batch*: the _async
forms and the host forms through a context) against tests/reads_pattern_oracle.py.  The anchored forms build their A operand from the patterns
(anchored_tables_kernel<PatternSets>): counts around the tile and the wave, (queries, offsets, k) with 1 .. 64 rows per query, start / interior / 3'
ranges, junk allow bits above k with several offsets (a table leak would give a neighbouring shift matches that do not exist), N at position 0 and at
k - 1, k = 32 with only position 31 constrained; ragged batches with lengths 0, k - 1, k, k + 3 and 150 under both anchors, and the headroom case of the
ragged layout (k = 32, an all-N pattern, every second read too short).  The whole-read forms are the exact forms' kernels instantiated for patterns:
read lengths with and without matrix-core rounds, query counts around the block of 16, duplicates, one query, ragged batches with reads of 1 .. 31 bases.
Identities with the exact twins on singletons, between the families; the host forms above the cutoff with several distinct patterns (an upload sized at 8
bytes per pattern would lose half of them), in one chunk and across two; a hipGraph replay after the patterns changed in place; a queue of mixed exact
and pattern calls; an N in a read latched for sync; the query limit; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 / +15 with
lowercase bases, packed words at 16-byte and 8-mod-16 offsets with junk pad bits.  Every comparison is exact equality; guard words and bytes surround
the outputs and the dist arrays start at odd byte offsets."""
import numpy as np
import pytest

import pattern_oracle as po
import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_batch_oracle as rb
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
OFFS = (0, 1, 7, 15)
TRIPLES = {"best": 1, "best2": 2, "anchored": 2, "best_batch": 1, "anchored_batch": 2}


def _methods(c):
    """the twenty _async methods, by (kind, family, packed)"""
    return {("pattern", "best", False): c.reads_pattern_best_async, ("pattern", "best", True): c.reads_pattern_best_packed_async,
            ("pattern", "best2", False): c.reads_pattern_best2_async, ("pattern", "best2", True): c.reads_pattern_best2_packed_async,
            ("pattern", "anchored", False): c.reads_pattern_anchored_async, ("pattern", "anchored", True): c.reads_pattern_anchored_packed_async,
            ("pattern", "best_batch", False): c.reads_pattern_best_batch_async, ("pattern", "best_batch", True): c.reads_pattern_best_batch_packed_async,
            ("pattern", "anchored_batch", False): c.reads_pattern_anchored_batch_async,
            ("pattern", "anchored_batch", True): c.reads_pattern_anchored_batch_packed_async,
            ("hdist", "best", False): c.reads_hdist_best_async, ("hdist", "best", True): c.reads_hdist_best_packed_async,
            ("hdist", "best2", False): c.reads_hdist_best2_async, ("hdist", "best2", True): c.reads_hdist_best2_packed_async,
            ("hdist", "anchored", False): c.reads_hdist_anchored_async, ("hdist", "anchored", True): c.reads_hdist_anchored_packed_async,
            ("hdist", "best_batch", False): c.reads_hdist_best_batch_async, ("hdist", "best_batch", True): c.reads_hdist_best_batch_packed_async,
            ("hdist", "anchored_batch", False): c.reads_hdist_anchored_batch_async, ("hdist", "anchored_batch", True): c.reads_hdist_anchored_batch_packed_async}


def _dev_queries(kind, queries):
    import torch
    if kind == "pattern":
        return torch.from_numpy(rp.as_patterns(queries).view(np.int32).copy()).to("cuda:0")
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


def _table_dev(tab):
    import torch
    return torch.from_numpy(np.asarray(tab, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero(np.any([g != w for g, w in zip(got, want)], axis=0))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


def _fixed(ctx, kind, family, s, read_len, count, k, queries, lo=0, hi=None, off=0, woff=0, forms=(False, True)):
    """the fixed-length _async forms (ASCII, packed) of a family on the same data: a list of their outputs, guards checked"""
    import torch
    dq, nq = _dev_queries(kind, queries), len(queries)
    kw = dict(pos_lo=lo, pos_hi=hi) if family == "anchored" else {}
    m = _methods(ctx)
    got, keep = [], []
    for packed in forms:
        keep.append(_words_dev(ro.pack_reads(s, read_len, count), woff) if packed else _ascii_dev(s, off))
        o = Out(count, TRIPLES[family])
        torch.cuda.synchronize()
        m[(kind, family, packed)](keep[-1][1], read_len, count, k, dq, nq, *o.ptrs(), **kw)
        got.append(o.read(ctx))
    return got


def _ragged(ctx, kind, family, s, offsets, k, queries, anchor="start", lo=0, hi=0, off=0, woff=0, forms=(False, True)):
    import torch
    dq, nq = _dev_queries(kind, queries), len(queries)
    offsets = np.asarray(offsets, dtype=np.uint64)
    count = offsets.size - 1
    kw = dict(pos_lo=lo, pos_hi=hi, anchor=anchor) if family == "anchored_batch" else {}
    m = _methods(ctx)
    d_off = _table_dev(offsets)
    got, keep = [], []
    for packed in forms:
        o = Out(count, TRIPLES[family])
        if packed:
            wtab = rb.word_offsets_of(offsets)
            keep.append((_words_dev(rb.pack_batch(s, offsets, seed=k), woff), _table_dev(wtab)))
            torch.cuda.synchronize()
            m[(kind, family, True)](keep[-1][0][1], keep[-1][1], d_off, count, int(wtab[-1]), k, dq, nq, *o.ptrs(), **kw)
        else:
            keep.append(_ascii_dev(s, off))
            torch.cuda.synchronize()
            m[(kind, family, False)](keep[-1][1], d_off, count, int(offsets[-1]), k, dq, nq, *o.ptrs(), **kw)
        got.append(o.read(ctx))
    return got


def _all_same(got, want, tag):
    for name, g in zip(("ascii", "packed"), got):
        assert _same(g, want), (name, tag, _diff(g, want))


def _random_patterns(rng, nq, k, junk=True):
    ps = np.stack([po.from_sets(po.random_sets(rng, k)) for _ in range(nq)])
    if junk and k < 32:
        ps = ps | (rng.integers(0, 2**32, size=ps.shape, dtype=np.uint64) << np.uint64(k)).astype(np.uint32)
    return np.ascontiguousarray(ps.astype(np.uint32))


def _instance(rng, pattern, k):
    out = np.zeros(k, dtype=np.int64)
    for i in range(k):
        ok = [c for c in range(4) if (int(pattern[c]) >> i) & 1]
        out[i] = rng.choice(ok) if ok else rng.integers(0, 4)
    return out


def _ascii(rng, codes):
    s = ro.LUT[codes].astype(np.uint8)
    s[rng.random(s.size) < 0.3] |= 0x20
    return s


def _fixed_reads(rng, read_len, count, k, patterns, plant=12):
    codes = rng.integers(0, 4, size=(count, read_len))
    for _ in range(plant if read_len >= k and len(patterns) else 0):
        r, i, q = rng.integers(0, count), rng.integers(0, read_len - k + 1), rng.integers(0, len(patterns))
        codes[r, i:i + k] = _instance(rng, patterns[q], k)
    return _ascii(rng, codes.reshape(-1))


def _ragged_reads(rng, lengths, k, patterns, plant=12):
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    long = [r for r, n in enumerate(lengths) if n >= k]
    for _ in range(plant if long and len(patterns) else 0):
        r, q = long[rng.integers(0, len(long))], rng.integers(0, len(patterns))
        i = int(off[r]) + rng.integers(0, lengths[r] - k + 1)
        codes[i:i + k] = _instance(rng, patterns[q], k)
    return _ascii(rng, codes), off


def _special(patterns, k):
    """in place: N at position 0 and at k - 1 (pattern 0); k == 32: only position 31 constrained (the last pattern)"""
    ones = np.uint32(0xFFFFFFFF if k == 32 else (1 << k) - 1)
    patterns[0] |= np.uint32(1) | np.uint32(1 << (k - 1))
    if k == 32:
        patterns[-1] = ones & np.uint32(0x7FFFFFFF)
        patterns[-1][2] = ones  # position 31: G only
    return patterns


def _ranges(read_len, k, offsets):
    last = read_len - k
    w = min(offsets, last + 1)
    return ((0, w - 1), ((last + 1 - w) // 2, (last + 1 - w) // 2 + w - 1), (last + 1 - w, None))  # start, interior, 3'


# ---- anchored, fixed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 33, 65))
@pytest.mark.parametrize("nq,offsets,k", ((1, 1, 16), (2, 4, 16), (17, 4, 17), (33, 1, 32), (3, 33, 32), (5, 16, 1)))
def test_anchored_fixed_shapes_ranges_and_junk_allow_bits(ctx, count, nq, offsets, k):
    rng = np.random.default_rng(1000 * count + 37 * nq + offsets)
    read_len = 100
    patterns = _special(_random_patterns(rng, nq, k), k)
    s = _fixed_reads(rng, read_len, count, k, patterns)
    for i, (lo, hi) in enumerate(_ranges(read_len, k, offsets)):
        want = rp.reads_anchored(s, read_len, count, k, patterns, lo, hi)
        _all_same(_fixed(ctx, "pattern", "anchored", s, read_len, count, k, patterns, lo, hi, off=OFFS[(i + count) % 4], woff=(i + nq) % 2), want, (lo, hi))


def test_anchored_tables_ignore_allow_bits_above_k(ctx):
    """every allow bit at positions >= k set, four and sixteen offsets: the rows of the shifts s > 0 read the entries behind 64 + k - 1, which must be
    zero; with a leak they would collect matches and report distances that are too small"""
    rng = np.random.default_rng(4)
    read_len, count = 80, 70
    for k, offsets in ((5, 4), (16, 16), (31, 4), (12, 33)):
        clean = _random_patterns(rng, 6, k, junk=False)
        junk = clean | np.uint32((0xFFFFFFFF << k) & 0xFFFFFFFF)
        s = _fixed_reads(rng, read_len, count, k, clean)
        for lo, hi in _ranges(read_len, k, offsets):
            want = rp.reads_anchored(s, read_len, count, k, clean, lo, hi)
            _all_same(_fixed(ctx, "pattern", "anchored", s, read_len, count, k, junk, lo, hi, off=7, woff=1), want, (k, lo, hi))


# ---- anchored, ragged --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,width,k", ((1, 1, 16), (3, 4, 16), (17, 4, 17), (33, 2, 32), (5, 16, 1), (2, 33, 32)))
def test_anchored_ragged_mixed_lengths_both_anchors(ctx, nq, width, k):
    rng = np.random.default_rng(2000 + 41 * nq + width)
    lengths = [0, k - 1, k, k + 3, 150] * 15 + [k + 1, k + width, 64, 1]
    rng.shuffle(lengths)
    patterns = _special(_random_patterns(rng, nq, k), k)
    s, off = _ragged_reads(rng, lengths, k, patterns)
    for anchor in ("start", "end"):
        for lo in (0, 2):
            want = rp.reads_anchored_batch(s, off, k, patterns, anchor, lo, lo + width - 1)
            _all_same(_ragged(ctx, "pattern", "anchored_batch", s, off, k, patterns, anchor, lo, lo + width - 1, off=OFFS[(nq + lo) % 4], woff=lo // 2), want,
                      (anchor, lo))


def test_the_ragged_layouts_headroom_an_all_n_pattern_at_k_32(ctx):
    """k = 32, an all-N pattern, four offsets, tiles of 32 reads in which every second read is too short for a window: its rows are inadmissible but live
    for its neighbours, start at 127 and collect 32 matches at every position -- they end at exactly 95, above every real distance.  The short reads get
    the fill, the others distance 0, query 0 and their lowest admissible offset."""
    k, width = 32, 4
    rng = np.random.default_rng(95)
    all_n = np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32)
    for nq in (1, 3):
        patterns = np.concatenate([all_n] * nq)
        for short in (31, 0, 20):
            lengths = [40 if r % 2 == 0 else short for r in range(64)] + [short, 90, short]
            s, off = _ragged_reads(rng, lengths, k, patterns, plant=0)
            long = np.array(lengths) >= k
            for anchor in ("start", "end"):
                first = np.where(long, 0 if anchor == "start" else np.array(lengths) - k - (width - 1), 0)
                want = rp.reads_anchored_batch(s, off, k, patterns, anchor, 0, width - 1)
                assert (want[2][long] == 0).all() and (want[0][long] == 0).all() and np.array_equal(want[1][long], first[long].astype(np.uint32))
                assert (want[2][~long] == 0xFF).all() and (want[0][~long] == rp.NO_U32).all() and (want[3][~long] == rp.NO_U32).all()
                _all_same(_ragged(ctx, "pattern", "anchored_batch", s, off, k, patterns, anchor, 0, width - 1, off=1, woff=1), want, (nq, short, anchor))


# ---- whole-read forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", (20, 33, 150))
@pytest.mark.parametrize("nq", (1, 15, 16, 17, 33))
def test_whole_read_best_and_best2(ctx, read_len, nq):
    rng = np.random.default_rng(3000 + read_len + nq)
    k = 16 if read_len > 20 else 12
    count = 301 if read_len == 150 else 1100
    patterns = _random_patterns(rng, nq, k)
    if nq > 1:
        patterns[nq - 1] = patterns[0]  # an equal pattern at the highest index: the runner-up wherever pattern 0 wins
    s = _fixed_reads(rng, read_len, count, k, patterns)
    s[2:2 + k] = ro.LUT[_instance(rng, patterns[0], k)]  # read 0 holds an instance of pattern 0 (and so of its twin), unless a set of it is empty
    want = rp.reads_best2(s, read_len, count, k, patterns)
    if nq > 1:
        won = want[0] == 0  # where pattern 0 wins its twin ties with it: the runner-up has the same distance
        assert np.array_equal(want[5][won], want[2][won]) and (want[2][0] > 0 or won[0])
    else:
        assert (want[3] == rp.NO_U32).all()
    _all_same(_fixed(ctx, "pattern", "best2", s, read_len, count, k, patterns, off=OFFS[nq % 4], woff=nq % 2), want, "best2")
    _all_same(_fixed(ctx, "pattern", "best", s, read_len, count, k, patterns, off=OFFS[(nq + 1) % 4], woff=(nq + 1) % 2), want[:3], "best")


@pytest.mark.parametrize("nq", (1, 16, 17, 33))
def test_whole_read_best_batch_with_short_reads_mixed_in(ctx, nq):
    """reads of 1 .. 31 bases among long ones: the ASCII kernel's exact one-window-per-thread path, here through QueryKind<PatternSets>"""
    rng = np.random.default_rng(3500 + nq)
    k = 9
    lengths = [int(x) for x in rng.integers(1, 32, size=120)] + [150] * 60 + [0, 33, 64, 2000]
    rng.shuffle(lengths)
    patterns = _random_patterns(rng, nq, k)
    s, off = _ragged_reads(rng, lengths, k, patterns)
    _all_same(_ragged(ctx, "pattern", "best_batch", s, off, k, patterns, off=OFFS[nq % 4], woff=nq % 2), rp.reads_best_batch(s, off, k, patterns), nq)
    lengths = [150] * 200  # and no short read at all: rounds only
    s, off = _ragged_reads(rng, lengths, k, patterns)
    _all_same(_ragged(ctx, "pattern", "best_batch", s, off, k, patterns, off=7, woff=1), rp.reads_best_batch(s, off, k, patterns), (nq, "long"))


# ---- identities --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 16, 31, 32))
def test_singletons_equal_the_exact_twins_in_every_family(ctx, k):
    rng = np.random.default_rng(4000 + k)
    queries = ro.random_queries(rng, 19, k)
    queries[11] = queries[4]
    single = rp.singletons(queries, k)
    read_len, count = 64, 333
    s = ro.random_reads(rng, read_len, count, k, queries)
    for family, lo, hi in (("best", 0, None), ("best2", 0, None), ("anchored", 3, 9), ("anchored", read_len - k, None)):
        a = _fixed(ctx, "pattern", family, s, read_len, count, k, single, lo, hi, off=1, woff=1)
        b = _fixed(ctx, "hdist", family, s, read_len, count, k, queries, lo, hi, off=1, woff=1)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), family
    lengths = [0, k - 1, k, k + 3, 150, 40] * 20
    sb, off = rb.random_batch(rng, lengths, k, queries)
    for family, anchor in (("best_batch", "start"), ("anchored_batch", "start"), ("anchored_batch", "end")):
        a = _ragged(ctx, "pattern", family, sb, off, k, single, anchor, 1, 4, off=7)
        b = _ragged(ctx, "hdist", family, sb, off, k, queries, anchor, 1, 4, off=7)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), (family, anchor)


@pytest.mark.parametrize("read_len", (32, 33, 64))
def test_best_is_best2s_first_triple_and_anchored_over_the_whole_read_is_best2(ctx, read_len):
    rng = np.random.default_rng(4500 + read_len)
    k, count, nq = 13, 500, 21
    patterns = _random_patterns(rng, nq, k)
    s = _fixed_reads(rng, read_len, count, k, patterns)
    two = _fixed(ctx, "pattern", "best2", s, read_len, count, k, patterns, off=15)
    one = _fixed(ctx, "pattern", "best", s, read_len, count, k, patterns, off=15)
    full = _fixed(ctx, "pattern", "anchored", s, read_len, count, k, patterns, 0, None, off=15)
    for j in (0, 1):
        assert _same(one[j], two[j][:3]) and _same(full[j], two[j]), j
    assert _same(two[0], rp.reads_best2(s, read_len, count, k, patterns))


# ---- host forms above the cutoff ---------------------------------------------------------------------------------------------------------------
def test_host_forms_through_the_context_upload_every_pattern(ctx):
    """all ten host forms through a context that runs everything on the GPU, five distinct patterns: one chunk.  The chunk loops copy the patterns to the
    device once, 16 bytes each"""
    rng = np.random.default_rng(5000)
    k, read_len, count = 14, 90, 700
    patterns = _random_patterns(rng, 5, k)
    s = _fixed_reads(rng, read_len, count, k, patterns, plant=60)
    words = ro.pack_reads(s, read_len, count)
    want = rp.reads_best2(s, read_len, count, k, patterns)
    assert len(set(want[0].tolist())) >= 4  # the later patterns win somewhere
    assert _same(ctx.reads_pattern_best(s, read_len, k, patterns), want[:3]) and _same(ctx.reads_pattern_best_packed(words, read_len, count, k, patterns), want[:3])
    assert _same(ctx.reads_pattern_best2(s, read_len, k, patterns), want) and _same(ctx.reads_pattern_best2_packed(words, read_len, count, k, patterns), want)
    wa = rp.reads_anchored(s, read_len, count, k, patterns, 70, None)
    assert _same(ctx.reads_pattern_anchored(s, read_len, k, patterns, pos_lo=70), wa)
    assert _same(ctx.reads_pattern_anchored_packed(words, read_len, count, k, patterns, pos_lo=70), wa)
    lengths = [0, k - 1, k, k + 3, 150, 33] * 100
    sb, off = _ragged_reads(rng, lengths, k, patterns, plant=60)
    wb, woff = rb.pack_batch(sb, off), rb.word_offsets_of(off)
    want = rp.reads_best_batch(sb, off, k, patterns)
    assert len(set(want[0].tolist())) >= 5
    assert _same(ctx.reads_pattern_best_batch(sb, off, k, patterns), want) and _same(ctx.reads_pattern_best_batch_packed(wb, woff, off, k, patterns), want)
    for anchor in ("start", "end"):
        want = rp.reads_anchored_batch(sb, off, k, patterns, anchor, 0, 3)
        assert _same(ctx.reads_pattern_anchored_batch(sb, off, k, patterns, pos_lo=0, pos_hi=3, anchor=anchor), want)
        assert _same(ctx.reads_pattern_anchored_batch_packed(wb, woff, off, k, patterns, pos_lo=0, pos_hi=3, anchor=anchor), want)


def test_host_anchored_forms_across_two_chunks():
    """900,000 reads of 150 bases, four offsets at the 3' end, three distinct patterns (10.8 * 10^6 offset-pattern pairs, above the default cutoff) on a
    context with the default dispatch: the ASCII form's chunks are 894,784 whole reads, the packed form's 838,860.  The oracle runs on the compacted
    spans.  (The other chunk loops: the two tests below.)"""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1783)
    read_len, count, k, w = 150, 900_000, 8, 3
    lo = read_len - k - w
    patterns = np.stack([po.from_iupac(x) for x in ("ACGTNNRY", "NNTTGGCA", "GGSWACNT")])
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    s = ro.LUT[codes].reshape(-1)
    s[::7] |= 0x20
    span = w + k
    compact = np.ascontiguousarray(s.reshape(count, read_len)[:, lo:]).reshape(-1)
    want = list(rp.reads_anchored(compact, span, count, k, patterns, 0, None))
    for i in (1, 4):
        want[i] = want[i] + np.uint32(lo)
    assert len(set(want[0].tolist())) == 3
    with bn.Context(0) as c:
        assert _same(c.reads_pattern_anchored(s, read_len, k, patterns, pos_lo=lo), want)
        words = ro.pack_reads(s, read_len, count)
        assert _same(c.reads_pattern_anchored_packed(words, read_len, count, k, patterns, pos_lo=lo), want)


CHUNK_PATTERNS = ("ACGTNNRYACGTWS", "NNTTGGCAWSACGT", "GGSWACNTKMTAAC")  # three distinct patterns, none a singleton list


def _ranges_around(count, pers, w=1200):
    """read ranges the oracle runs on: the head, the tail and w reads on both sides of every chunk boundary"""
    return [(0, w), (count - w, count)] + [(per - w, per + w) for per in pers]


def test_host_whole_read_forms_across_two_chunks(ctx):
    """reads_host_loop and reads_host_loop2 with pattern queries over a chunk boundary: 900,000 reads of 150 bases; the ASCII forms' chunks are
    894,784 whole reads (128 Mi bytes / 150), the packed forms' 838,860 (4 Mi words / 5).  The reads on both sides of each boundary hold a planted
    instance of a pattern at their last, first and an interior window.  The oracle runs on the reads around both boundaries, on the head and on the
    tail; every other read is compared with one-chunk runs of the same form on the two parts (which the tests above check against the oracle): a wrong
    output offset, or patterns lost between the chunks, shows in either.  Then an N past the boundary reports its absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1784)
    read_len, count, k = 150, 900_000, 14
    per_ascii, per_packed = (128 << 20) // read_len, ((128 << 20) // 32) // 5
    assert per_packed < per_ascii < count
    patterns = np.stack([po.from_iupac(x) for x in CHUNK_PATTERNS])
    codes = rng.integers(0, 4, size=(count, read_len), dtype=np.uint8)
    for per in (per_ascii, per_packed):
        codes[per - 1, read_len - k:] = _instance(rng, patterns[0], k)  # the last window of the chunk's last read
        codes[per, :k] = _instance(rng, patterns[1], k)                  # the first window of the next chunk's first read
        codes[per + 1, 60:60 + k] = _instance(rng, patterns[2], k)
    s = ro.LUT[codes.reshape(-1)]
    del codes
    s[::7] |= 0x20
    words = ctx.encode_fixed(s, read_len).reshape(-1)  # (the library's own fixed-length encoder: zero pad bits)
    wpr = 5
    got = {"ascii": ctx.reads_pattern_best2(s, read_len, k, patterns), "packed": ctx.reads_pattern_best2_packed(words, read_len, count, k, patterns),
           "ascii1": ctx.reads_pattern_best(s, read_len, k, patterns), "packed1": ctx.reads_pattern_best_packed(words, read_len, count, k, patterns)}
    for a, b in _ranges_around(count, (per_ascii, per_packed)):
        want = rp.reads_best2(s[a * read_len:b * read_len], read_len, b - a, k, patterns)
        for name, g in got.items():
            part = tuple(x[a:b] for x in g)
            assert _same(part, want[:len(part)]), (name, a, b, _diff(part, want[:len(part)]))
    for per in (per_ascii, per_packed):
        assert [int(got["ascii"][2][r]) for r in (per - 1, per, per + 1)] == [0, 0, 0]  # the planted instances are found
    assert len(set(got["ascii"][0].tolist())) == 3
    # every read: the two parts on their own, one chunk each
    lo, hi = s[:per_ascii * read_len], s[per_ascii * read_len:]
    parts = ctx.reads_pattern_best2(lo, read_len, k, patterns), ctx.reads_pattern_best2(hi, read_len, k, patterns)
    whole = tuple(np.concatenate([a, b]) for a, b in zip(*parts))
    assert _same(got["ascii"], whole) and _same(got["ascii1"], whole[:3])
    lo, hi = words[:per_packed * wpr], words[per_packed * wpr:]
    parts = (ctx.reads_pattern_best2_packed(lo, read_len, per_packed, k, patterns), ctx.reads_pattern_best2_packed(hi, read_len, count - per_packed, k, patterns))
    whole = tuple(np.concatenate([a, b]) for a, b in zip(*parts))
    assert _same(got["packed"], whole) and _same(got["packed1"], whole[:3]) and _same(got["packed"], got["ascii"])
    bad_at = per_ascii * read_len + 99
    s[bad_at] = ord("N")
    for fn in (ctx.reads_pattern_best, ctx.reads_pattern_best2):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(s, read_len, k, patterns)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei


def test_host_ragged_forms_across_two_chunks(ctx):
    """reads_batch_host_loop and anchored_batch_host_loop with pattern queries over a chunk boundary: 900,000 reads of 100 .. 200 bases (about 135 M
    bases); the ASCII forms' first chunk is the longest run of whole reads within 128 Mi bytes, the packed forms' within 4 Mi words, each later chunk
    with rebased tables.  Planted instances at the last window of the chunk's last read and at the first and last windows of the next chunk's first
    read.  Checked as the test above: the oracle around the boundaries, on the head and the tail, one-chunk runs of the two parts everywhere."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1785)
    count, k = 900_000, 14
    lengths = rng.integers(100, 201, size=count)
    off = rb.offsets_of(lengths)
    wo = rb.word_offsets_of(off)
    per_ascii = int(np.searchsorted(off, 128 << 20, side="right")) - 1  # the chunk budget: the largest r1 with off[r1] <= 128 Mi
    per_packed = int(np.searchsorted(wo, (128 << 20) // 32, side="right")) - 1
    assert 0 < per_packed < per_ascii < count
    patterns = np.stack([po.from_iupac(x) for x in CHUNK_PATTERNS])
    codes = rng.integers(0, 4, size=int(off[-1]), dtype=np.uint8)
    for per in (per_ascii, per_packed):
        b, b1 = int(off[per]), int(off[per + 1])
        codes[b - k:b] = _instance(rng, patterns[0], k)    # the last window of the chunk's last read
        codes[b:b + k] = _instance(rng, patterns[1], k)    # the first window of the next chunk's first read
        codes[b1 - k:b1] = _instance(rng, patterns[2], k)  # and its last
    s = rb.LUT[codes]
    del codes
    s[::7] |= 0x20
    words, ewo = ctx.encode_batch(s, off)  # (the library's own ragged encoder: zero pad bits)
    assert np.array_equal(ewo, wo)
    kw = dict(pos_lo=0, pos_hi=3, anchor="end")
    got = {"best": ctx.reads_pattern_best_batch(s, off, k, patterns), "best packed": ctx.reads_pattern_best_batch_packed(words, wo, off, k, patterns),
           "anchored": ctx.reads_pattern_anchored_batch(s, off, k, patterns, **kw),
           "anchored packed": ctx.reads_pattern_anchored_batch_packed(words, wo, off, k, patterns, **kw)}
    for a, b in _ranges_around(count, (per_ascii, per_packed)):
        sub, tab = s[int(off[a]):int(off[b])], off[a:b + 1] - off[a]
        wants = {"best": rp.reads_best_batch(sub, tab, k, patterns), "anchored": rp.reads_anchored_batch(sub, tab, k, patterns, "end", 0, 3)}
        for name, g in got.items():
            part, want = tuple(x[a:b] for x in g), wants[name.split()[0]]
            assert _same(part, want), (name, a, b, _diff(part, want))
    for per in (per_ascii, per_packed):
        assert [int(got["best"][2][r]) for r in (per - 1, per)] == [0, 0] and [int(got["anchored"][2][r]) for r in (per - 1, per)] == [0, 0]
    assert len(set(got["best"][0].tolist())) == 3 and len(set(got["anchored"][0].tolist())) == 3

    def joined(parts):
        return tuple(np.concatenate([x, y]) for x, y in zip(*parts))
    p, cut = per_ascii, int(off[per_ascii])
    tabs = off[:p + 1], off[p:] - off[p]
    assert _same(got["best"], joined([ctx.reads_pattern_best_batch(s[:cut], tabs[0], k, patterns), ctx.reads_pattern_best_batch(s[cut:], tabs[1], k, patterns)]))
    assert _same(got["anchored"], joined([ctx.reads_pattern_anchored_batch(s[:cut], tabs[0], k, patterns, **kw),
                                          ctx.reads_pattern_anchored_batch(s[cut:], tabs[1], k, patterns, **kw)]))
    p, cut = per_packed, int(wo[per_packed])
    tabs, wtabs = (off[:p + 1], off[p:] - off[p]), (wo[:p + 1], wo[p:] - wo[p])
    assert _same(got["best packed"], joined([ctx.reads_pattern_best_batch_packed(words[:cut], wtabs[0], tabs[0], k, patterns),
                                             ctx.reads_pattern_best_batch_packed(words[cut:], wtabs[1], tabs[1], k, patterns)]))
    assert _same(got["anchored packed"], joined([ctx.reads_pattern_anchored_batch_packed(words[:cut], wtabs[0], tabs[0], k, patterns, **kw),
                                                 ctx.reads_pattern_anchored_batch_packed(words[cut:], wtabs[1], tabs[1], k, patterns, **kw)]))
    assert _same(got["best packed"], got["best"]) and _same(got["anchored packed"], got["anchored"])
    bad_at = int(off[per_ascii + 1]) - 2  # past the boundary, inside the END span of that read
    s[bad_at] = ord("N")
    for fn, more in ((ctx.reads_pattern_best_batch, {}), (ctx.reads_pattern_anchored_batch, kw)):
        with pytest.raises(bn.NucleotideError) as ei:
            fn(s, off, k, patterns, **more)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei


# ---- queues, graphs, errors -----------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_patterns_changed_in_place():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    read_len, count, k, nq = 151, 1500, 20, 33
    p1, p2 = _random_patterns(rng, nq, k), _random_patterns(rng, nq, k)
    s = _fixed_reads(rng, read_len, count, k, np.concatenate([p1, p2]), plant=200)
    wa1, wa2 = rp.reads_anchored(s, read_len, count, k, p1, 0, 3), rp.reads_anchored(s, read_len, count, k, p2, 0, 3)
    wb1, wb2 = rp.reads_best2(s, read_len, count, k, p1), rp.reads_best2(s, read_len, count, k, p2)
    assert not np.array_equal(wa1[0], wa2[0]) and not np.array_equal(wb1[0], wb2[0])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s, 7)
        tw, wptr = _words_dev(ro.pack_reads(s, read_len, count), 1)
        dq = _dev_queries("pattern", p1)
        oa, ob = Out(count), Out(count)

        def enqueue():
            c.reads_pattern_anchored_packed_async(wptr, read_len, count, k, dq, nq, *oa.ptrs(), pos_lo=0, pos_hi=3)
            c.reads_pattern_best2_async(ptr, read_len, count, k, dq, nq, *ob.ptrs())
        enqueue()  # warm-up outside the capture: sizes the scratch
        assert _same(oa.read(c), wa1) and _same(ob.read(c), wb1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                enqueue()
            dq.copy_(_dev_queries("pattern", p2))
            for _ in range(2):
                oa.reset()
                ob.reset()
                g.replay()
                assert _same(oa.read(c), wa2) and _same(ob.read(c), wb2)
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_of_exact_and_pattern_calls_with_one_sync(ctx):
    """exact and pattern calls of all five families in turn on one context, different (count, n_queries) between consecutive calls (context scratch is
    laid out anew by each), one sync at the end"""
    import torch
    rng = np.random.default_rng(809)
    k, read_len = 15, 120
    m = _methods(ctx)
    jobs = []
    shapes = ((500, 5), (40, 33), (900, 1), (333, 17), (90, 40), (700, 16), (7, 2), (800, 3), (64, 20), (1000, 7))
    for i, (count, nq) in enumerate(shapes):
        family = ("anchored", "best2", "best_batch", "anchored_batch", "best")[i % 5]
        kind = "pattern" if (i // 5 + i) % 2 == 0 else "hdist"
        queries = ro.random_queries(rng, nq, k)
        patterns = _random_patterns(rng, nq, k) if kind == "pattern" else rp.singletons(queries, k)
        s = _fixed_reads(rng, read_len, count, k, patterns)
        off = rb.offsets_of([read_len] * count)
        jobs.append(dict(family=family, kind=kind, count=count, nq=nq, patterns=patterns, s=s, off=off, data=_ascii_dev(s, OFFS[i % 4]), tab=_table_dev(off),
                         dq=_dev_queries(kind, patterns if kind == "pattern" else queries), out=Out(count, TRIPLES[family])))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        fn, ptr, o = m[(j["kind"], j["family"], False)], j["data"][1], j["out"]
        if j["family"] in ("best", "best2"):
            fn(ptr, read_len, j["count"], k, j["dq"], j["nq"], *o.ptrs())
        elif j["family"] == "anchored":
            fn(ptr, read_len, j["count"], k, j["dq"], j["nq"], *o.ptrs(), pos_lo=100, pos_hi=None)
        elif j["family"] == "best_batch":
            fn(ptr, j["tab"], j["count"], j["s"].size, k, j["dq"], j["nq"], *o.ptrs())
        else:
            fn(ptr, j["tab"], j["count"], j["s"].size, k, j["dq"], j["nq"], *o.ptrs(), pos_lo=0, pos_hi=5, anchor="end")
    ctx.sync()  # the only sync of the queue
    for i, j in enumerate(jobs):
        a = (j["s"], read_len, j["count"], k, j["patterns"])
        want = {"best": lambda: rp.reads_best2(*a)[:3], "best2": lambda: rp.reads_best2(*a), "anchored": lambda: rp.reads_anchored(*a, 100, None),
                "best_batch": lambda: rp.reads_best_batch(j["s"], j["off"], k, j["patterns"]),
                "anchored_batch": lambda: rp.reads_anchored_batch(j["s"], j["off"], k, j["patterns"], "end", 0, 5)}[j["family"]]()
        got = j["out"].read()
        assert _same(got, want), (i, j["family"], j["kind"], _diff(got, want))


def test_an_n_in_a_read_is_latched_for_sync(ctx):
    """an all-N pattern does not make an N in a read valid: the whole-read forms validate every byte, the anchored forms their spans' bytes"""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, read_len, count = 17, 150, 400
    patterns = np.concatenate([np.full((1, 4), (1 << k) - 1, dtype=np.uint32), _random_patterns(rng, 4, k)])
    s = _fixed_reads(rng, read_len, count, k, patterns)
    off = _table_dev(rb.offsets_of([read_len] * count))
    dq, nq = _dev_queries("pattern", patterns), len(patterns)
    bad_at = 150 * 200 + 140
    b = s.copy()
    b[bad_at] = ord("N")
    b[bad_at + 150 * 3] = ord("x")  # a later one
    t, ptr = _ascii_dev(b, 3)
    m = _methods(ctx)
    calls = (("best", lambda o: m[("pattern", "best", False)](ptr, read_len, count, k, dq, nq, *o.ptrs()), True),
             ("best2", lambda o: m[("pattern", "best2", False)](ptr, read_len, count, k, dq, nq, *o.ptrs()), True),
             ("best_batch", lambda o: m[("pattern", "best_batch", False)](ptr, off, count, s.size, k, dq, nq, *o.ptrs()), True),
             ("anchored", lambda o: m[("pattern", "anchored", False)](ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=129, pos_hi=None), True),
             ("anchored_batch", lambda o: m[("pattern", "anchored_batch", False)](ptr, off, count, s.size, k, dq, nq, *o.ptrs(), pos_lo=0, pos_hi=4, anchor="end"), True),
             ("anchored", lambda o: m[("pattern", "anchored", False)](ptr, read_len, count, k, dq, nq, *o.ptrs(), pos_lo=0, pos_hi=4), False))  # outside the spans
    for family, call, fails in calls:
        o = Out(count, TRIPLES[family])
        torch.cuda.synchronize()
        call(o)
        if fails:
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at), family
            del ei
            ctx.sync()  # latched once
        else:
            assert _same(o.read(ctx), rp.reads_anchored(s, read_len, count, k, patterns, 0, 4))


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES patterns on 64 reads: the anchored form with two offsets and the whole-read best2, against the host form in slices of 256
    merged by reads_best2_oracle.merge_top2; one more pattern is Unsupported"""
    import bitnuc_amd as bn
    from bitnuc_amd import api
    rng = np.random.default_rng(65537)
    k, read_len, count, nq = 12, 60, 64, 65536
    patterns = rp.singletons(ro.random_queries(rng, nq, k), k)
    patterns[:, 0] |= np.uint32(1 << 5)  # position 5 also admits A: no longer singletons
    s = _fixed_reads(rng, read_len, count, k, patterns[60000:], plant=8)
    free = api.context_free()
    assert _same(free.reads_pattern_anchored(s, read_len, k, patterns[:64], pos_lo=47), rp.reads_anchored(s, read_len, count, k, patterns[:64], 47, None))
    full = r2.merge_top2([(i, free.reads_pattern_anchored(s, read_len, k, patterns[i:i + 256], pos_lo=47)) for i in range(0, nq, 256)])
    _all_same(_fixed(ctx, "pattern", "anchored", s, read_len, count, k, patterns, 47, None, off=1, woff=1), full, "anchored")
    full = r2.merge_top2([(i, free.reads_pattern_best2(s, read_len, k, patterns[i:i + 256])) for i in range(0, nq, 256)])
    _all_same(_fixed(ctx, "pattern", "best2", s, read_len, count, k, patterns, off=1, woff=1), full, "best2")
    more = np.concatenate([patterns, patterns[:1]])
    dq = _dev_queries("pattern", more)
    o = Out(count)
    t, ptr = _ascii_dev(s, 0)
    with pytest.raises(bn.NucleotideError):
        ctx.reads_pattern_anchored_async(ptr, read_len, count, k, dq, nq + 1, *o.ptrs(), pos_lo=47, pos_hi=None)
    o.read(ctx)  # nothing was written: the guards and the fill pattern are checked by the next assertion
    assert all(bool((a == FILL32).all()) for a in o.w)


def test_cpp_mirror_of_the_pattern_forms(ctx, tmp_path):
    """the ten reads_pattern_* methods of include/bitnuc.hpp against a brute force, via tests/cpp/test_reads_pattern_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_reads_pattern_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_reads_pattern_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_seeded_differential_fuzz(ctx):
    """60 seeded cases over the five families: random k, pattern counts, lengths, ranges and alignments"""
    rng = np.random.default_rng(0xF022)
    for case in range(60):
        family = ("best", "best2", "anchored", "best_batch", "anchored_batch")[case % 5]
        k = int(rng.integers(1, 33))
        nq = int(rng.choice([1, 2, 3, 16, 17, 40]))
        patterns = _random_patterns(rng, nq, k)
        off, woff = OFFS[int(rng.integers(0, 4))], int(rng.integers(0, 2))
        if family in ("best", "best2", "anchored"):
            read_len, count = int(rng.integers(k, 160)), int(rng.integers(1, 400))
            s = _fixed_reads(rng, read_len, count, k, patterns)
            if family == "anchored":
                last = read_len - k
                lo = int(rng.integers(0, last + 1))
                hi = min(last, lo + int(rng.integers(0, 64 - k + 1)))
                want = rp.reads_anchored(s, read_len, count, k, patterns, lo, hi)
                got = _fixed(ctx, "pattern", family, s, read_len, count, k, patterns, lo, hi, off=off, woff=woff)
            else:
                want = rp.reads_best2(s, read_len, count, k, patterns)[:3 * TRIPLES[family]]
                got = _fixed(ctx, "pattern", family, s, read_len, count, k, patterns, off=off, woff=woff)
        else:
            lengths = [int(x) for x in rng.integers(0, 200, size=int(rng.integers(1, 300)))]
            s, offs = _ragged_reads(rng, lengths, k, patterns)
            if int(offs[-1]) == 0:
                continue
            if family == "anchored_batch":
                anchor, lo = ("start", "end")[int(rng.integers(0, 2))], int(rng.integers(0, 20))
                hi = lo + int(rng.integers(0, 64 - k + 1))
                want = rp.reads_anchored_batch(s, offs, k, patterns, anchor, lo, hi)
                got = _ragged(ctx, "pattern", family, s, offs, k, patterns, anchor, lo, hi, off=off, woff=woff)
            else:
                want = rp.reads_best_batch(s, offs, k, patterns)
                got = _ragged(ctx, "pattern", family, s, offs, k, patterns, off=off, woff=woff)
        _all_same(got, want, (case, family, k, nq))
