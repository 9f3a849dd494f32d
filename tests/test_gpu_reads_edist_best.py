"""GPU tests of the indel-tolerant best match per read over the WHOLE read (bitnuc_reads_edist_best[_packed]_async, _best_batch[_packed]_async, the pattern
twins and the host forms above the cutoff; reads_edist_best_kernel, scan_edist_best_device.h) against tests/reads_edist_best_oracle.py (the plain DP over
the whole read).  One read per lane; the lane walks its read in pieces of 64 bases and carries the columns of four queries from piece to piece; the ragged
layout runs the loop wave-uniformly over the longest read of the wave with Eq forced to 0 behind a lane's own length, a wave of equal lengths takes the
unmasked loop.  So: counts around the wave and the block and one beyond the bounded grid; lengths around the pieces; one read of 100,000 bases whose only
match ends past base 65,536; waves whose 64 lanes all have different lengths (0 and lengths below k included), waves of equal lengths and a wave without
any window; k in {1, 16, 31, 32}; Q around the interleave factor and at the limit; the planted and overhang cases of the host test on both layouts with the
bytes behind the batch included; invalid bytes at a piece's first and last byte and (unreported) in a read shorter than k; NULL second pointers; argument
errors; a hipGraph replay after lengths, reads and queries changed; a queue mixed with reads_edist_anchored_async and reads_hdist_best_batch_async; the
host forms in one chunk and across two; the bitnuc.hpp methods; the header's identities; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 /
+15 with lowercase bases and packed words at 16-byte and 8-mod-16 offsets with junk pad bits run on the same data.  Every comparison is exact equality of
all written arrays; guard words and bytes surround all six outputs and both dist arrays start at odd byte offsets."""
import numpy as np
import pytest

import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_best_oracle as bo
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
OFFS = (0, 1, 7, 15)
MAX_READ = 1 << 26
Q16 = np.array([0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 1, 3])  # ACGTAACCGGTTAGCT
FAR16 = np.array([3] * 15 + [2])


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _dev_queries(queries, pattern=False):
    import torch
    if pattern:
        return torch.from_numpy(rp.as_patterns(queries).view(np.int32).copy()).to("cuda:0")
    return _dev_u64(np.asarray(queries, dtype=np.uint64).reshape(-1))


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


def _ascii_dev(s, off, behind=None):
    """s at byte offset `off` of a device buffer; `behind`: the bytes right behind the batch (default zeros: invalid, must never be examined)"""
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    if behind is not None:
        t[off + s.size:off + s.size + len(behind)] = torch.from_numpy(np.asarray(behind, dtype=np.uint8))
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


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def _fns(ctx, pattern, ragged):
    name = "reads_" + ("pattern_" if pattern else "") + "edist_best" + ("_batch" if ragged else "")
    return getattr(ctx, name + "_async"), getattr(ctx, name + "_packed_async")


def _ragged(ctx, s, off, k, queries, aoff=0, woff=0, words=None, behind=None, pattern=False, triples=2):
    """(the outputs of the ragged ASCII form, of the ragged packed form), guards checked"""
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count, nq = off.size - 1, len(queries)
    wtab = rb.word_offsets_of(off)
    w = rb.pack_batch(s, off, seed=k) if words is None else words
    t, ptr = _ascii_dev(s, aoff, behind)
    tw, wptr = _words_dev(w, woff)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_queries(queries, pattern)
    o1, o2 = Out(count, triples), Out(count, triples)
    fa, fp = _fns(ctx, pattern, True)
    torch.cuda.synchronize()
    fa(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs())
    fp(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o2.ptrs())
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _fixed(ctx, s, n, count, k, queries, aoff=0, woff=0, words=None, behind=None, pattern=False, triples=2):
    import torch
    nq = len(queries)
    w = ro.pack_reads(s, n, count) if words is None else words
    t, ptr = _ascii_dev(s[:n * count], aoff, behind)
    tw, wptr = _words_dev(w, woff)
    dq = _dev_queries(queries, pattern)
    o1, o2 = Out(count, triples), Out(count, triples)
    fa, fp = _fns(ctx, pattern, False)
    torch.cuda.synchronize()
    fa(ptr, n, count, k, dq, nq, *o1.ptrs())
    fp(wptr, n, count, k, dq, nq, *o2.ptrs())
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check_ragged(ctx, s, off, k, queries, want=None, tag=(), pattern=False, **kw):
    if want is None:
        want = (bo.reads_pattern_edist_best_batch if pattern else bo.reads_edist_best_batch)(s, off, k, queries)
    a, p = _ragged(ctx, s, off, k, queries, pattern=pattern, **kw)
    assert _same(a, want), ("ragged ascii", tag, _diff(a, want))
    assert _same(p, want), ("ragged packed", tag, _diff(p, want))
    return want


def _check_fixed(ctx, s, n, count, k, queries, want=None, tag=(), pattern=False, **kw):
    if want is None:
        want = (bo.reads_pattern_edist_best if pattern else bo.reads_edist_best)(s, n, count, k, queries)
    a, p = _fixed(ctx, s, n, count, k, queries, pattern=pattern, **kw)
    assert _same(a, want), ("fixed ascii", tag, _diff(a, want))
    assert _same(p, want), ("fixed packed", tag, _diff(p, want))
    return want


def _check_both(ctx, s, n, count, k, queries, tag=(), i=0, **kw):
    """equal lengths: the fixed and the ragged layout on the same data"""
    want = _check_fixed(ctx, s, n, count, k, queries, tag=tag, aoff=OFFS[i % 4], woff=i % 2, **kw)
    _check_ragged(ctx, s, rb.offsets_of([n] * count), k, queries, want=want, tag=tag, aoff=OFFS[(i + 1) % 4], woff=(i + 1) % 2, **kw)
    return want


def _plant(rng, s, off, k, queries, share=0.8, cap=400):
    """a copy of a query with 1 .. 3 edits, at least one of them an indel, anywhere inside about `share` of the reads of at least k + 3 bases"""
    o = np.asarray(off).astype(np.int64)
    lens = np.diff(o)
    rows = np.nonzero(lens >= k + 3)[0]
    if rows.size > cap:
        rows = rng.choice(rows, size=cap, replace=False)
    for r in rows:
        if rng.random() >= share:
            continue
        c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, len(queries)))], k), int(rng.integers(1, 4)))
        at = int(o[r]) + int(rng.integers(0, int(lens[r]) - len(c) + 1))
        s[at:at + len(c)] = _ascii(c) | (s[at:at + len(c)] & 0x20)


def _random(rng, lengths, k, nq, plant=True):
    queries = ro.random_queries(rng, nq, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    if plant:
        _plant(rng, s, off, k, queries)
    return queries, s, off


def _wave_lengths(rng, count, k, top=150):
    """waves of 64 consecutive reads with 64 different lengths each: 0, k - 1, k, 63, 64, 65, 127, 128, 129 and others up to `top`"""
    out = []
    must = sorted({0, max(k - 1, 0), k, 63, 64, 65, 127, 128, 129})
    while len(out) < count:
        rest = [x for x in rng.permutation(top + 1) if x not in must][:64 - len(must)]
        wave = must + [int(x) for x in rest]
        rng.shuffle(wave)
        out += wave
    return out[:count]


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 257])
def test_counts_around_the_wave_and_the_block(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, nq) in enumerate(((16, 9), (31, 3), (1, 5))):
        queries, s, off = _random(rng, _wave_lengths(rng, count, k), k, nq)
        _check_ragged(ctx, s, off, k, queries, aoff=OFFS[(i + count) % 4], woff=(i + count) % 2, tag=(count, k))
        n = (65, 150, 64)[i]
        queries, s, off = _random(rng, [n] * count, k, nq)
        _check_both(ctx, s, n, count, k, queries, tag=(count, k, n), i=i + count)


def test_a_count_beyond_the_bounded_grid(ctx):
    """one read more than the grid has lanes (8 workgroups of 256 lanes per CU): one lane walks two reads; reads of k + 1 bases"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 1
    rng = np.random.default_rng(5)
    k, nq = 6, 3
    queries = ro.random_queries(rng, nq, k)
    s = ro.LUT[rng.integers(0, 4, size=count * (k + 1))].astype(np.uint8)
    want = _check_fixed(ctx, s, k + 1, count, k, queries, aoff=1, woff=1)
    lengths = np.full(count, k + 1)
    lengths[-1], lengths[0] = k, k + 2  # (the same total: a ragged batch whose last read, the second of lane 0, differs)
    off = rb.offsets_of(lengths)
    _check_ragged(ctx, s, off, k, queries, aoff=7, woff=0)
    assert (want[2] <= k).all()


@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_lengths_around_the_pieces_on_both_layouts(ctx, k):
    rng = np.random.default_rng(200 + k)
    for i, n in enumerate((max(k, 1), 63, 64, 65, 127, 128, 129, 150, 257)):
        if n < k:
            continue
        queries, s, off = _random(rng, [n] * 70, k, 5)
        _check_both(ctx, s, n, 70, k, queries, tag=(k, n), i=i)


def test_one_read_of_100000_bases_whose_only_match_ends_past_base_65536(ctx):
    rng = np.random.default_rng(31)
    k, n = 16, 100_000
    codes = np.full(n, 2, dtype=np.int64)  # a run of G: Q16 never aligns with it cheaply
    codes[70_001:70_016] = np.delete(Q16, 5)
    s = _ascii(codes)
    queries = np.array([ro.word_of(FAR16), ro.word_of(Q16), ro.word_of(FAR16[::-1])], dtype=np.uint64)
    want = bo.six_of_columns(*bo.long_read_columns(codes, k, rp.singletons(queries, k)))
    assert tuple(int(a[0]) for a in want[:3]) == (1, 70_016, 1)
    _check_fixed(ctx, s, n, 1, k, queries, want=want, aoff=1, woff=1)
    # ragged: the long read in a wave of short ones (the masked loop runs 100,000 steps for every lane)
    short = ro.LUT[rng.integers(0, 4, size=300)].astype(np.uint8)
    lengths = [100, n, 15, 0, 185]
    b = np.concatenate([short[:100], s, short[100:115], short[115:300]])
    off = rb.offsets_of(lengths)
    w = bo.reads_edist_best_batch(np.concatenate([short[:100], short[100:]]), rb.offsets_of([100, 0, 15, 0, 185]), k, queries)
    w = tuple(np.concatenate([a[:1], x, a[2:]]) for a, x in zip(w, want))
    _check_ragged(ctx, b, off, k, queries, want=w, aoff=7, woff=0)


@pytest.mark.parametrize("k", [1, 16, 32])
def test_ragged_waves_all_different_all_equal_and_without_a_window(ctx, k):
    rng = np.random.default_rng(300 + k)
    lengths = _wave_lengths(rng, 64, k)                                  # wave 0: 64 different lengths
    lengths += [130] * 64                                                # wave 1: equal lengths, the unmasked loop
    lengths += [int(x) for x in rng.integers(0, k, size=64)]             # wave 2: no window at all
    lengths += [k] * 64                                                  # wave 3: equal, one piece
    lengths += _wave_lengths(rng, 40, k, top=300)
    queries, s, off = _random(rng, lengths, k, 7)
    want = _check_ragged(ctx, s, off, k, queries, aoff=15, woff=1)
    assert (want[2][128:192] == 255).all()


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 8, 9, 33])
def test_queries_around_the_interleave_factor(ctx, nq):
    rng = np.random.default_rng(400 + nq)
    k = 16
    queries, s, off = _random(rng, _wave_lengths(rng, 96, k), k, nq)
    _check_ragged(ctx, s, off, k, queries, aoff=OFFS[nq % 4], woff=nq % 2)
    queries, s, off = _random(rng, [129] * 66, k, nq)
    _check_both(ctx, s, 129, 66, k, queries, i=nq)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries on a handful of short reads (the winner planted at the last index, its duplicate in the middle); one more is refused"""
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(65537)
    k, nq = 20, 65536  # (k = 20: no random query comes within one edit of a read)
    queries = ro.random_queries(rng, nq, k)
    queries[30000] = queries[nq - 1] ^ (np.uint64(1) << np.uint64(60))
    lengths = [28, 70, 19, 20]
    codes = rng.integers(0, 4, size=sum(lengths))
    codes[5:5 + k - 1] = np.delete(ro.query_codes(queries[nq - 1], k), 4)
    codes[28 + 40:28 + 40 + k] = ro.query_codes(queries[77], k)
    s = _ascii(codes)
    off = rb.offsets_of(lengths)
    want = _check_ragged(ctx, s, off, k, queries, aoff=1, woff=1)
    assert tuple(int(a[0]) for a in want) == (30000, 5 + k - 1, 1, nq - 1, 5 + k - 1, 1) and tuple(int(a[1]) for a in want[:3]) == (77, 60, 0)
    assert int(want[2][2]) == 255
    o = Out(4)
    t, ptr = _ascii_dev(s, 0)
    d_off = _dev_u64(off)
    dq = _dev_queries(np.zeros(nq + 1, dtype=np.uint64))
    assert _raw_err(ctx, "_batch", (ptr, d_off.data_ptr(), 4, int(off[-1])), k, dq, nq + 1, o.ptrs()) == (L.UNSUPPORTED, nq + 1)
    assert _raw_err(ctx, "", (ptr, 28, 1), k, dq, nq + 1, o.ptrs()) == (L.UNSUPPORTED, nq + 1)
    ctx.sync()
    assert o.untouched()


# ---- 2. the cases ----------------------------------------------------------------------------------------------------------------------------

def test_planted_reads_dist_and_end_by_hand(ctx):
    """the host test's planted reads: a deletion straddling bases 60 .. 70, an insertion across 127 | 128, a copy ending at the last base, a copy at base 0"""
    n = 257
    reads = np.full((4, n), 2, dtype=np.int64)
    reads[0, 58:73] = np.delete(Q16, 5)
    reads[1, 120:137] = np.insert(Q16, 8, 3)
    reads[2, n - 16:] = Q16
    reads[3, :16] = Q16
    s = _ascii(reads.reshape(-1))
    queries = np.array([ro.word_of(FAR16), ro.word_of(Q16)], dtype=np.uint64)
    want = _check_both(ctx, s, n, 4, 16, queries, behind=_ascii(Q16))
    assert [(int(d), int(e)) for d, e in zip(want[2], want[1])] == [(1, 73), (1, 137), (0, 257), (0, 16)]


def test_the_overhang_traps(ctx):
    """a copy completed by the next read, the previous read, the packed pad bits or the bytes behind the batch must not score 0"""
    k = 16
    lengths = [70, 74, 70, 40, 130, 10]
    codes = [np.full(n, 2, dtype=np.int64) for n in lengths]
    codes[1][-10:] = Q16[:10]
    codes[2][:6] = Q16[10:]
    codes[3][-6:] = Q16[:6]
    codes[4][:10] = Q16[6:]
    codes[4][-10:] = Q16[:10]
    codes[5][:6] = Q16[10:]           # a read shorter than k completing its neighbour's copy
    s = _ascii(np.concatenate(codes))
    off = rb.offsets_of(lengths)
    queries = np.array([ro.word_of(Q16)], dtype=np.uint64)
    words = rb.pack_batch(s, off, pad_codes={1: list(Q16[10:]), 3: list(Q16[6:]), 4: list(Q16[10:])})
    want = _check_ragged(ctx, s, off, k, queries, words=words, aoff=1, woff=1)
    assert (want[2][:5] > 0).all() and int(want[2][5]) == 255
    n = 74
    f = np.full((3, n), 2, dtype=np.int64)
    f[0, -10:] = Q16[:10]
    f[1, :6] = Q16[10:]
    f[2, -10:] = Q16[:10]              # completed by the bytes behind the batch
    s = _ascii(f.reshape(-1))
    pad = np.full((3, 96 - n), 2, dtype=np.int64)
    pad[0, :6] = pad[2, :6] = Q16[10:]
    want = _check_both(ctx, s, n, 3, k, queries, words=None, behind=_ascii(Q16[10:]))
    a, p = _fixed(ctx, s, n, 3, k, queries, words=ro.pack_reads(s, n, 3, pad_codes=pad), behind=_ascii(Q16[10:]), aoff=7)
    assert _same(a, want) and _same(p, want) and (want[2] > 0).all()


def test_ties_duplicates_patterns_and_fills(ctx):
    k, n = 16, 200
    codes = np.full(n, 2, dtype=np.int64)
    codes[30:46] = Q16
    codes[140:156] = Q16
    s = _ascii(codes)
    qw = ro.word_of(Q16)
    queries = np.array([ro.word_of(FAR16), qw, qw], dtype=np.uint64)
    want = _check_both(ctx, s, n, 1, k, queries)
    assert [int(a[0]) for a in want] == [1, 46, 0, 2, 46, 0]
    want = _check_both(ctx, s, n, 1, k, queries[1:2])
    assert [int(a[0]) for a in want] == [0, 46, 0, 0xFFFFFFFF, 0xFFFFFFFF, 255]
    rng = np.random.default_rng(9)
    for kk in (1, 16, 32):
        q2, b, off = _random(rng, [kk, 70, 0, 129, max(kk - 1, 0), 64, 257], kk, 2)
        ones = (1 << kk) - 1
        sing = rp.singletons(q2, kk)
        pats = np.stack([np.zeros(4, dtype=np.uint32), sing[0], np.array([ones] * 4, dtype=np.uint32), sing[1]])
        _check_ragged(ctx, b, off, kk, pats, pattern=True, aoff=7)
        _check_ragged(ctx, b, off, kk, sing, want=bo.reads_edist_best_batch(b, off, kk, q2), pattern=True)  # singletons equal the exact form
    # fills from the host-known arguments
    import torch
    dq = _dev_queries(queries)
    for kk, nq, rl in ((0, 3, 200), (16, 0, 200), (16, 3, 15)):
        o = Out(1)
        t, ptr = _ascii_dev(s, 0)
        torch.cuda.synchronize()
        ctx.reads_edist_best_async(ptr, rl, 1, kk, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), eo.fill6(1))
        o = Out(1)
        ctx.reads_edist_best_batch_async(ptr, _dev_u64([0, rl]), 1, rl, kk, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), eo.fill6(1))


def test_null_second_pointers_write_the_best_triple_only(ctx):
    rng = np.random.default_rng(41)
    k = 17
    queries, s, off = _random(rng, _wave_lengths(rng, 130, k), k, 6)
    want = bo.reads_edist_best_batch(s, off, k, queries)
    a, p = _ragged(ctx, s, off, k, queries, triples=1, aoff=1)
    assert _same(a, want[:3]) and _same(p, want[:3])
    queries, s, off = _random(rng, [100] * 70, k, 6)
    want = bo.reads_edist_best(s, 100, 70, k, queries)
    a, p = _fixed(ctx, s, 100, 70, k, queries, triples=1, woff=1)
    assert _same(a, want[:3]) and _same(p, want[:3])


def _raw_err(ctx, form, head, k, dq, nq, six, pattern=False, packed=False):
    """(status, value) of a device call through the raw entry point; form: "" (fixed) or "_batch" """
    import ctypes as C
    from bitnuc_amd import _lib as L
    raw = getattr(L.load(), "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_best" + form + ("_packed" if packed else "") + "_async")
    nptr = (1 if form == "" else (3 if packed else 2))
    err = L.BitnucErr()
    st = raw(ctx._h, *(C.c_void_p(p) if i < nptr else p for i, p in enumerate(head)), k, C.c_void_p(dq.data_ptr()), nq,
             *(C.c_void_p(p) if p else None for p in six), C.byref(err))
    return st, int(err.value)


def test_argument_errors_in_their_order_leave_the_outputs_untouched(ctx):
    import torch
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(2)
    k, count = 12, 100
    queries, s, off = _random(rng, rng.integers(0, 150, size=count), k, 16)
    total = int(off[-1])
    wtab = rb.word_offsets_of(off)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 0)
    d_off, d_wtab = _dev_u64(off), _dev_u64(wtab)
    o = Out(count)
    six = o.ptrs()
    torch.cuda.synchronize()
    for pattern in (False, True):
        dq = _dev_queries(rp.singletons(queries, k) if pattern else queries, pattern)
        for packed, head in ((False, (ptr, d_off.data_ptr(), count, total)), (True, (wptr, d_wtab.data_ptr(), d_off.data_ptr(), count, int(wtab[-1])))):
            def err(head, k_, nq, six_):
                return _raw_err(ctx, "_batch", head, k_, dq, nq, six_, pattern, packed)
            assert err(head, 33, 65537, six) == (L.SEQUENCE_TOO_LONG, 33)                 # k first
            big = head[:-1] + (2**58 if not packed else 2**53,)
            assert err(big, k, 65537, six) == (L.UNSUPPORTED, big[-1])                     # then the totals' limit
            assert err(head, k, 65537, six) == (L.UNSUPPORTED, 65537)                      # the query count
            for bad in ((six[0], six[1], six[2], 0, six[4], six[5]), (six[0], six[1], six[2], six[3], 0, 0), (six[0], six[1], six[2], six[3] + 2, six[4], six[5]),
                        (six[0], 0, six[2], six[3], six[4], six[5])):
                assert err(head, k, 16, bad) == (L.UNSUPPORTED, 0)
            for i in ((1,) if not packed else (1, 2)):  # a table NULL or not 8-byte aligned
                for v in (0, head[i] + 4):
                    assert err(head[:i] + (v,) + head[i + 1:], k, 16, six) == (L.UNSUPPORTED, 0)
            assert err((0,) + head[1:], k, 16, six) == (L.UNSUPPORTED, 0)                  # the data, last
            if packed:
                assert err((wptr + 4,) + head[1:], k, 16, six) == (L.UNSUPPORTED, 0)
        for packed, p0 in ((False, ptr), (True, wptr)):
            def ferr(head, k_, nq, six_):
                return _raw_err(ctx, "", head, k_, dq, nq, six_, pattern, packed)
            assert ferr((p0, 2**32 - 1, 1), 33, 65537, six) == (L.SEQUENCE_TOO_LONG, 33)
            assert ferr((p0, 2**32 - 1, 1), k, 65537, six) == (L.UNSUPPORTED, 2**32 - 1)   # the read_len / count limits
            assert ferr((p0, MAX_READ + 1, 1), k, 65537, six) == (L.UNSUPPORTED, 65537)    # the query count
            assert ferr((p0, MAX_READ + 1, 0), k, 16, six) == (L.UNSUPPORTED, MAX_READ + 1)  # a read above 2^26 bases, before count == 0
            assert ferr((p0, 64, 0), k, 16, (0,) * 6) == (L.OK, 0)                         # count == 0
            assert ferr((p0, 64, 4), k, 16, (six[0], six[1], six[2], six[3], six[4], 0)) == (L.UNSUPPORTED, 0)
            assert ferr((p0, 64, 4), k, 16, (six[0], six[1] + 2, six[2], six[3], six[4], six[5])) == (L.UNSUPPORTED, 0)
            assert ferr((0, 64, 4), k, 16, six) == (L.UNSUPPORTED, 0)                      # the data, last
    ctx.sync()
    assert o.untouched()


def test_invalid_bytes_at_a_pieces_first_and_last_byte_and_in_a_read_shorter_than_k(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, nq = 17, 9
    lengths = [150, 16, 200, 0, 3, 129, 64, 16]
    queries, s, off = _random(rng, lengths, k, nq)
    o_ = [int(x) for x in off]
    count = len(lengths)
    want = bo.reads_edist_best_batch(s, off, k, queries)
    dq, d_off = _dev_queries(queries), _dev_u64(off)
    b = s.copy()
    for r in (1, 4, 7):
        b[o_[r]:o_[r + 1]] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=lengths[r])  # every byte of the reads shorter than k
    for aoff in (0, 3):
        t, ptr = _ascii_dev(b, aoff)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_best_batch_async(ptr, d_off, count, o_[-1], k, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), want)  # no error, correct results
    # a piece's first byte (base 64 of read 2), a piece's last byte (base 127 of read 5), a read's last byte (read 6, base 63), the batch's first byte
    for bad_at, later, aoff in ((o_[2] + 64, o_[5] + 5, 0), (o_[5] + 127, o_[6] + 1, 9), (o_[6] + 63, None, 5), (0, o_[2] + 128, 1)):
        c = b.copy()
        c[bad_at] = ord("N")
        if later is not None:
            c[later] = ord("x")  # a later one: the first in buffer order wins
        t, ptr = _ascii_dev(c, aoff)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_best_batch_async(ptr, d_off, count, o_[-1], k, dq, nq, *o.ptrs())
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing is left for the next sync
    # the fixed layout: reads of 129 bases, an N at the last byte of the last read and an earlier one at a piece's first byte
    n, cnt = 129, 5
    q2, f, _ = _random(rng, [n] * cnt, k, nq)
    f[4 * n + 128] = ord("N")
    f[2 * n + 64] = ord("n")
    t, ptr = _ascii_dev(f, 7)
    o = Out(cnt)
    torch.cuda.synchronize()
    ctx.reads_edist_best_async(ptr, n, cnt, k, _dev_queries(q2), nq, *o.ptrs())
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.sync()
    assert (ei.value.byte, ei.value.index) == (ord("n"), 2 * n + 64)
    del ei
    t2, ptr2 = _ascii_dev(b, 1)  # the next call on the same context is clean and correct
    o = Out(count)
    torch.cuda.synchronize()
    ctx.reads_edist_best_batch_async(ptr2, d_off, count, o_[-1], k, dq, nq, *o.ptrs())
    assert _same(o.read(ctx), want)


def test_graph_replay_after_the_lengths_the_reads_and_the_queries_changed():
    """the tables are read on the device at every replay: the same count and totals, other lengths, reads and queries give the new answers"""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    k, nq, count = 31, 9, 640
    l1 = np.array(_wave_lengths(rng, count, k))
    l1[(l1 % 32 == 0) & (l1 > 0)] += 1  # no multiple of 32: a permutation then keeps the words' total as well
    l2 = rng.permutation(l1)
    (q1, s1, off1), (q2, s2, off2) = _random(rng, l1, k, nq), _random(rng, l2, k, nq)
    w1tab, w2tab = rb.word_offsets_of(off1), rb.word_offsets_of(off2)
    assert int(off1[-1]) == int(off2[-1]) and int(w1tab[-1]) == int(w2tab[-1]) and not np.array_equal(off1, off2)
    want1, want2 = bo.reads_edist_best_batch(s1, off1, k, q1), bo.reads_edist_best_batch(s2, off2, k, q2)
    n = 129
    qf1, f1, _ = _random(rng, [n] * 100, k, nq)
    qf2, f2, _ = _random(rng, [n] * 100, k, nq)
    wantf2 = bo.reads_edist_best(f2, n, 100, k, q2)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = rb.pack_batch(s1, off1)
        tw, wptr = _words_dev(w, 1)
        tf, fptr = _ascii_dev(f1, 1)
        dq, d_off, d_wtab = _dev_queries(q1), _dev_u64(off1), _dev_u64(w1tab)
        o1, o2, o3 = Out(count), Out(count), Out(100)

        def run():
            c.reads_edist_best_batch_async(ptr, d_off, count, int(off1[-1]), k, dq, nq, *o1.ptrs())
            c.reads_edist_best_batch_packed_async(wptr, d_wtab, d_off, count, int(w1tab[-1]), k, dq, nq, *o2.ptrs())
            c.reads_edist_best_async(fptr, n, 100, k, dq, nq, *o3.ptrs())
        run()  # warm-up outside the capture: sizes the scratch
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1) and _same(o3.read(c), bo.reads_edist_best(f1, n, 100, k, q1))
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                run()
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(rb.pack_batch(s2, off2).view(np.int64)).to(tw.device)
            tf[1:1 + f2.size] = torch.from_numpy(f2).to(tf.device)
            dq.copy_(_dev_queries(q2))
            d_off.copy_(_dev_u64(off2))
            d_wtab.copy_(_dev_u64(w2tab))
            o1.reset(), o2.reset(), o3.reset()
            g.replay()
            assert _same(o1.read(c), want2) and _same(o2.read(c), want2) and _same(o3.read(c), wantf2)
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_with_one_sync(ctx):
    """the whole-read edit-distance calls (all eight _async forms in turn) between reads_edist_anchored_async and reads_hdist_best_batch_async calls on one
    context, different (count, n_queries) between consecutive calls (all lay out scratch 10 anew), one sync at the end, every result checked afterwards"""
    import torch
    rng = np.random.default_rng(809)
    k, n = 21, 64
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (700, 1), (333, 17), (90, 40), (600, 16), (7, 2), (300, 3))):
        ragged = i % 2 == 1
        lengths = rng.integers(0, 150, size=count) if ragged else np.full(count, n)
        queries, s, off = _random(rng, lengths, k, nq)
        wtab = rb.word_offsets_of(off)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, off=off, wtab=wtab, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         dp=_dev_queries(rp.singletons(queries, k), True), d_off=_dev_u64(off), d_wtab=_dev_u64(wtab), out=Out(count), ham=Out(count, 1), anch=Out(count),
                         wdev=_words_dev(rb.pack_batch(s, off), i & 1), ragged=ragged))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, ptr, dq, dp = j["i"], j["count"], j["nq"], j["ascii"][1], j["dq"], j["dp"]
        total, wtotal, wptr = int(j["off"][-1]), int(j["wtab"][-1]), j["wdev"][1]
        form = i // 2 % 4
        if j["ragged"]:
            if form == 0:
                ctx.reads_edist_best_batch_async(ptr, j["d_off"], count, total, k, dq, nq, *j["out"].ptrs())
            elif form == 1:
                ctx.reads_edist_best_batch_packed_async(wptr, j["d_wtab"], j["d_off"], count, wtotal, k, dq, nq, *j["out"].ptrs())
            elif form == 2:
                ctx.reads_pattern_edist_best_batch_async(ptr, j["d_off"], count, total, k, dp, nq, *j["out"].ptrs())
            else:
                ctx.reads_pattern_edist_best_batch_packed_async(wptr, j["d_wtab"], j["d_off"], count, wtotal, k, dp, nq, *j["out"].ptrs())
        else:  # (a fixed batch of 64-base reads: its packed words are two per read in either layout)
            if form == 0:
                ctx.reads_edist_best_async(ptr, n, count, k, dq, nq, *j["out"].ptrs())
            elif form == 1:
                ctx.reads_edist_best_packed_async(wptr, n, count, k, dq, nq, *j["out"].ptrs())
            elif form == 2:
                ctx.reads_pattern_edist_best_async(ptr, n, count, k, dp, nq, *j["out"].ptrs())
            else:
                ctx.reads_pattern_edist_best_packed_async(wptr, n, count, k, dp, nq, *j["out"].ptrs())
            ctx.reads_edist_anchored_async(ptr, n, count, k, dq, nq, *j["anch"].ptrs(), pos_lo=0, pos_hi=None)
        ctx.reads_hdist_best_batch_async(ptr, j["d_off"], count, total, k, dq, nq, *j["ham"].ptrs())
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, s, off, queries = j["i"], j["s"], j["off"], j["queries"]
        want = bo.reads_edist_best_batch(s, off, k, queries)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        ham = j["ham"].read()
        assert _same(ham, rb.batch_best(s, off, k, queries)), i
        assert (got[2] <= ham[2]).all()  # never above the whole-read Hamming best
        if not j["ragged"]:
            assert _same(j["anch"].read(), got), i  # reads of at most 64 bases: the anchored form over the whole read, byte for byte


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """900,000 reads of 150 bases (135 * 10^6 bases: two chunks of the ASCII form, whose first holds 128 Mi / 150 reads; the packed form's chunks are cut
    at 4 Mi words / 5), k = 16, two queries, on a context with the default dispatch; the reads on both sides of each boundary hold a planted winner.  The
    oracle runs on the reads around the boundaries, the first and the last ones; everywhere else the two-chunk results must equal the _async form's on the
    whole batch.  20,000 reads run in one chunk.  Then an N past the boundary reports its absolute index."""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    count, n, k = 900_000, 150, 16
    per_ascii, per_packed = (128 << 20) // n, ((128 << 20) // 32) // 5
    assert 0 < per_packed < per_ascii < count
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=count * n, dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    for per in (per_ascii, per_packed):
        codes[per * n - k:per * n] = qc[0]                              # the chunk's last read: query 0 in its last k bases
        codes[per * n:per * n + k] = qc[1]                              # the next chunk's first read: query 1 at base 0
        codes[(per + 1) * n + 60:(per + 1) * n + 60 + k - 1] = np.delete(qc[0], 4)
    s = ro.LUT[codes]
    del codes
    rows = np.unique(np.concatenate([np.arange(200), np.arange(count - 200, count)] + [np.arange(per - 100, per + 100) for per in (per_ascii, per_packed)]))
    sample = np.ascontiguousarray(s.reshape(count, n)[rows]).reshape(-1)
    want = bo.reads_edist_best(sample, n, rows.size, k, queries)
    for per in (per_ascii, per_packed):
        at = int(np.searchsorted(rows, per))
        assert [tuple(int(a[r]) for a in want[:3]) for r in (at - 1, at)] == [(0, n, 0), (1, k, 0)] and int(want[2][at + 1]) <= 1
    c = bn.Context(0)
    try:
        words = ro.pack_reads(s, n, count)
        t, ptr = _ascii_dev(s, 0)
        o = Out(count)
        torch.cuda.synchronize()
        c.reads_edist_best_async(ptr, n, count, k, _dev_queries(queries), 2, *o.ptrs())
        dev = o.read(c)
        del t, o
        assert _same(tuple(a[rows] for a in dev), want)
        off = rb.offsets_of([n] * count)
        for got in (c.reads_edist_best(s, n, k, queries), c.reads_edist_best_packed(words, n, count, k, queries),
                    c.reads_pattern_edist_best_packed(words, n, count, k, rp.singletons(queries, k)), c.reads_edist_best_batch(s, off, k, queries),
                    c.reads_edist_best_batch_packed(words, rb.word_offsets_of(off), off, k, queries)):
            assert _same(tuple(a[rows] for a in got), want), _diff(tuple(a[rows] for a in got), want)
            assert _same(got, dev)
        m = 20_000  # 6 * 10^6 base-query pairs: one chunk through the device
        assert _same(c.reads_edist_best(s[:m * n], n, k, queries), tuple(a[:m] for a in dev))
        assert _same(c.reads_pattern_edist_best_batch(s[:m * n], off[:m + 1], k, rp.singletons(queries, k), second=False), tuple(a[:m] for a in dev[:3]))
        bad_at = (per_ascii + 1) * n + 149
        s[bad_at] = ord("N")
        for call in (lambda: c.reads_edist_best(s, n, k, queries), lambda: c.reads_edist_best_batch(s, off, k, queries)):
            with pytest.raises(bn.NucleotideError) as ei:
                call()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
            del ei
    finally:
        c.close()


def test_cpp_mirror_of_the_whole_read_edist_forms(ctx, tmp_path):
    """the eight reads_*edist_best* methods of include/bitnuc.hpp against the plain DP, via tests/cpp/test_reads_edist_best_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_reads_edist_best_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_reads_edist_best_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ---- 3. identities ---------------------------------------------------------------------------------------------------------------------------

def test_identities_on_the_device(ctx):
    """reads of at most 64 bases equal the anchored form over the whole read; a ragged batch of equal lengths equals the fixed form (_check_both, everywhere
    above); singleton patterns equal the exact form; never above the whole-read Hamming best; truncation never lowers best_dist"""
    import torch
    rng = np.random.default_rng(55)
    k, count = 16, 300
    for n in (16, 33, 64):
        queries, s, off = _random(rng, [n] * count, k, 6)
        t, ptr = _ascii_dev(s, 1)
        tw, wptr = _words_dev(ro.pack_reads(s, n, count), 1)
        dq = _dev_queries(queries)
        o = [Out(count) for _ in range(4)]
        torch.cuda.synchronize()
        ctx.reads_edist_best_async(ptr, n, count, k, dq, 6, *o[0].ptrs())
        ctx.reads_edist_anchored_async(ptr, n, count, k, dq, 6, *o[1].ptrs(), pos_lo=0, pos_hi=None)
        ctx.reads_edist_best_packed_async(wptr, n, count, k, dq, 6, *o[2].ptrs())
        ctx.reads_edist_anchored_packed_async(wptr, n, count, k, dq, 6, *o[3].ptrs(), pos_lo=0, pos_hi=None)
        ctx.sync()
        got = [x.read() for x in o]
        assert _same(got[0], got[1]) and _same(got[2], got[3]) and _same(got[0], got[2]), n
    n = 150
    queries, s, off = _random(rng, [n] * count, k, 6)
    want = _check_both(ctx, s, n, count, k, queries)
    _check_fixed(ctx, s, n, count, k, rp.singletons(queries, k), want=want, pattern=True, aoff=15)
    ham = bo.hamming_best_dist(s, off, k, queries)
    assert (want[2] <= ham).all() and (want[2] < ham).any()
    for m in (k, 63, 64, 65, 128, 149):
        cut = np.ascontiguousarray(s.reshape(count, n)[:, :m]).reshape(-1)
        a, p = _fixed(ctx, cut, m, count, k, queries)
        assert _same(a, p) and (a[2] >= want[2]).all(), m


# ---- 4. fuzz ---------------------------------------------------------------------------------------------------------------------------------

def test_seeded_differential_fuzz(ctx):
    """150 seeded cases, each a ragged batch of 24 reads of six different lengths and, of its longest length, the fixed batch.  k in 12 .. 32: with shorter
    queries a random read of 100 bases holds a window within a mismatch or two of some query by chance, and the third requirement below could not be
    asked of every case.  The inputs are checked on the oracles alone, in every case: at least one read's best alignment crosses a 64-base boundary (its
    last k - dist bases, which every alignment of that distance holds, lie on both sides of one); at least one read is shorter than k; the edit distance
    is strictly below the whole-read Hamming best in at least a quarter of the reads with a window."""
    for seed in range(150):
        rng = np.random.default_rng(0xF022 + seed)
        k, nq = int(rng.integers(12, 33)), int(rng.integers(1, 10))
        distinct = [int(rng.integers(0, k)), int(rng.integers(k, 64)), int(rng.integers(64 + k, 141)), int(rng.integers(64 + k, 141)), int(rng.integers(k, 141)),
                    int(rng.integers(k, 141))]
        lengths = [distinct[i % 6] for i in rng.permutation(24)]
        queries = ro.random_queries(rng, nq, k)
        s, off = rb.random_batch(rng, lengths, k, queries, plant=0)
        o_ = off.astype(np.int64)
        for r, n in enumerate(lengths):
            if n < k + 1:
                continue
            qc = ro.query_codes(queries[int(rng.integers(0, nq))], k)
            c = np.delete(qc, int(rng.integers(3, k - 3))) if r % 3 else np.insert(qc, int(rng.integers(3, k - 3)), int(rng.integers(0, 4)))
            c = c[:n]
            at = 64 - len(c) // 2 if n >= 64 + k and r % 2 == 0 else int(rng.integers(0, n - len(c) + 1))  # straddling base 64, or anywhere
            s[o_[r] + at:o_[r] + at + len(c)] = _ascii(c) | (s[o_[r] + at:o_[r] + at + len(c)] & 0x20)
        want = bo.reads_edist_best_batch(s, off, k, queries)
        lens = np.diff(o_)
        has = lens >= k
        d, e = want[2].astype(np.int64), want[1].astype(np.int64)
        crosses = has & ((e - (k - d)) // 64 < (e - 1) // 64) & (k - d >= 2)
        ham = bo.hamming_best_dist(s, off, k, queries)
        assert crosses.any() and (~has).any() and 4 * int((d[has] < ham[has]).sum()) >= int(has.sum()), (seed, k, nq)
        a, p = _ragged(ctx, s, off, k, queries, aoff=OFFS[seed % 4], woff=seed % 2)
        assert _same(a, want), (seed, "ascii", _diff(a, want))
        assert _same(p, want), (seed, "packed", _diff(p, want))
        if seed % 5 == 0:
            n = max(lengths)
            rows = [r for r in range(24) if lengths[r] == n]
            f = np.concatenate([s[o_[r]:o_[r + 1]] for r in rows])
            _check_fixed(ctx, f, n, len(rows), k, queries, want=tuple(a[rows] for a in want), aoff=OFFS[(seed + 1) % 4], woff=(seed + 1) % 2, tag=seed)
