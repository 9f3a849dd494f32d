"""GPU tests of the indel-tolerant hit list (bitnuc_kmer_edist_hits* and its pattern twins; scan_edist_hits_device.h) against kmer_edist_oracle.ends(), the
plain DP: pos = nonzero(e <= tau) + 1, dist = e[pos - 1]; every comparison is exact equality.

C = the chunk of ends a lane owns (one entry of the scan), a wave's seam at 64 C, a workgroup's at 256 C.  Sizes 1, k, C - 1 .. C + 2k + 1, 64 C +- 1,
256 C +- 1 for k in {1, 2, 15, 16, 17, 31, 32} at tau in {0, 2, k}, ASCII at four byte offsets and packed words at both alignments, with *n_hits held
against the count (Q = 1) and the best match at every point; cap in {0, 1, total - 1, total, total + 1} with and without hit_dist and every end a hit;
bulges and exact copies at the seams (each hit once: none from the lane whose lead-in covers it, none missing); chunks without hits (waves with one
non-empty lane, waves with none, every second chunk empty); the scan's tile seam in chunk units; the host forms above the cutoff in one chunk and
across the host chunk boundary with cap inside the first chunk and spanning the boundary; one packed case past 2^32 bases, which also crosses the
grid's round of 2^29 bases; invalid bytes; patterns; a hipGraph replay; a queue mixed with Hamming hit lists, the best match and the count with one
sync; a seeded fuzz; the bitnuc.hpp mirror.  Guard words and bytes behind min(cap, total) everywhere."""
import ctypes as C_

import numpy as np
import pytest

import kmer_edist_hits_oracle as ho
import kmer_edist_oracle as ko
import pattern_oracle as po

pytestmark = pytest.mark.gpu

C = 1024   # kEdistRefChunk in bitnuc_amd/csrc/scan_edist_ref_device.h: the ends one lane owns per round, and one entry of the scan
WAVE = 64 * C
GROUP = 256 * C  # kEdistRefBlock lanes
TILE = 4096  # kHitsTile in scan_hits_device.h: entries per workgroup of the tile scan
KS = (1, 2, 15, 16, 17, 31, 32)
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _ascii(codes, rng=None):
    s = LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)
    if rng is not None:
        s[rng.random(s.size) < 0.3] |= 0x20  # about 30 % lowercase
    return s


def _query(rng, k):
    """a random query with junk above 2k"""
    return int(rng.integers(0, 2**63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))


def _qcodes(q, k):
    return np.array([(int(q) >> (2 * b)) & 3 for b in range(k)], dtype=np.int64)


def _word(codes):
    return sum(int(c) << (2 * b) for b, c in enumerate(codes))


def _with_insert(rng, qc, d):
    """the query's codes with d random bases inserted after position k / 2"""
    h = len(qc) // 2
    return np.concatenate([qc[:h], rng.integers(0, 4, size=d), qc[h:]])


def _text(rng, n, k, q, copies=4):
    """n random codes with edited copies of the query planted where they fit: exact, one deletion, one insertion, one substitution"""
    codes = rng.integers(0, 4, size=n)
    for i in range(copies):
        c = _qcodes(q, k)
        if i % 4 == 1 and k > 2:
            c = np.delete(c, int(rng.integers(0, k)))
        elif i % 4 == 2:
            c = np.insert(c, int(rng.integers(0, k)), int(rng.integers(0, 4)))
        elif i % 4 == 3:
            c[int(rng.integers(0, k))] ^= 1
        if len(c) <= n:
            p = int(rng.integers(0, n - len(c) + 1))
            codes[p:p + len(c)] = c
    return codes


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).to("cuda:0")


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


class Out:
    """device outputs: end (cap entries + guard words), hit_dist (cap bytes at byte offset 1 of a guarded buffer), n_hits between two guard words"""

    def __init__(self, cap, with_dist=True):
        import torch
        self.cap = cap
        self.with_dist = with_dist
        self.end = torch.full((cap + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
        self.dbuf = torch.full((1 + cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
        self.nbuf = torch.full((3,), FILL, dtype=torch.int64, device="cuda:0")

    def args(self):
        """(d_end, d_hit_dist, cap, d_n_hits)"""
        return (self.end if self.cap else None, (self.dbuf.data_ptr() + 1) if (self.with_dist and self.cap) else None, self.cap, self.nbuf.data_ptr() + 8)

    def refill(self):
        self.end.fill_(FILL)
        self.dbuf.fill_(0x5A)
        self.nbuf.fill_(FILL)

    def read(self, ctx):
        """(total, end[0 .. m), dist[0 .. m)) with m = min(cap, total), after a sync; nothing else may be written"""
        ctx.sync()
        nb = self.nbuf.cpu().numpy().view(np.uint64)
        assert nb[0] == np.uint64(FILL) and nb[2] == np.uint64(FILL), "written beside n_hits"
        total = int(nb[1])
        m = min(self.cap, total)
        e = self.end.cpu().numpy().view(np.uint64)
        d = self.dbuf.cpu().numpy()
        assert (e[m:] == np.uint64(FILL)).all(), "end written at or beyond min(cap, total)"
        if self.with_dist:
            assert d[0] == 0x5A and (d[1 + m:] == 0x5A).all(), "hit_dist written outside [0, min(cap, total))"
        else:
            assert (d == 0x5A).all(), "hit_dist written although NULL"
        return total, e[:m].copy(), d[1:1 + m].copy()


def _form(ctx, layout, pattern):
    return getattr(ctx, "kmer_" + ("pattern_" if pattern else "") + "edist_hits" + ("" if layout == "ascii" else "_packed") + "_async")


class Ref:
    """a reference on the device in both layouts"""

    def __init__(self, codes, off=0, woff=0, rng=None, layouts=("ascii", "packed")):
        self.n = len(codes)
        self.heads = {}
        self.keep = []
        if "ascii" in layouts:
            t, ptr = _ascii_dev(_ascii(codes, rng), off)
            self.keep.append(t)
            self.heads["ascii"] = (ptr, self.n)
        if "packed" in layouts:
            w = po.pack_codes(codes, junk=0xDEADBEEFCAFEF00D)
            t, ptr = _words_dev(w, woff)
            assert ptr % 16 == 8 * woff
            self.keep.append(t)
            self.heads["packed"] = (ptr, w.size, self.n)


def _hits(ctx, ref, layout, k, query, tau, cap, pattern=False, with_dist=True):
    """(total, end, dist) of one device form, guards checked; query: an exact word, or a (4,) pattern with pattern=True"""
    import torch
    o = Out(cap, with_dist)
    torch.cuda.synchronize()
    _form(ctx, layout, pattern)(*ref.heads[layout], k, query, int(tau), *o.args())
    return o.read(ctx)


def _check(got, want, cap, what, with_dist=True):
    pos, dist = want
    m = min(cap, pos.size)
    assert got[0] == pos.size, (what, "n_hits", got[0], pos.size)
    assert np.array_equal(got[1], pos[:m]), (what, "end", list(got[1][:6]), list(pos[:6]))
    if with_dist:
        assert np.array_equal(got[2], dist[:m]), (what, "hit_dist", list(got[2][:6]), list(dist[:6]))


def _both(ctx, codes, k, q, tau, what, off=0, woff=0, rng=None, pattern=None, want=None, slack=50):
    """both layouts with cap = total + slack against the DP; returns the expected (pos, dist)"""
    p = po.from_2bit(q, k) if pattern is None else pattern
    want = ho.hits(codes, k, p, tau) if want is None else want
    ref = Ref(codes, off, woff, rng)
    for layout in ("ascii", "packed"):
        _check(_hits(ctx, ref, layout, k, q if pattern is None else pattern, tau, want[0].size + slack, pattern is not None), want, want[0].size + slack,
               (what, layout))
    return want


def _sizes(k):
    return sorted({1, k} | set(range(C - 1, C + 2 * k + 2)) | {WAVE - 1, WAVE + 1, GROUP - 1, GROUP + 1})


def _count1(ctx, ref, layout, k, q, tau):
    import torch
    dq = _dev(np.array([q & (2**64 - 1)], dtype=np.uint64), np.int64)
    dt = _dev(np.array([min(tau, 2**32 - 1)], dtype=np.uint32), np.int32)
    out = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fn = ctx.kmer_edist_count_multi_async if layout == "ascii" else ctx.kmer_edist_count_multi_packed_async
    fn(*ref.heads[layout], k, dq, dt, 1, out)
    ctx.sync()
    return int(out.cpu().numpy().view(np.uint64)[0])


def _best1(ctx, ref, layout, k, q):
    import torch
    dq = _dev(np.array([q & (2**64 - 1)], dtype=np.uint64), np.int64)
    e = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    fn = ctx.kmer_edist_best_async if layout == "ascii" else ctx.kmer_edist_best_packed_async
    fn(*ref.heads[layout], k, dq, 1, e, d)
    ctx.sync()
    return int(e.cpu().numpy().view(np.uint64)[0]), int(d.cpu()[0])


# ---- 1. sizes, k, tau and alignments; 10. consistency with the count and the best match at every point ------------------------------------
@pytest.mark.parametrize("k", KS)
def test_sizes_around_the_chunk_the_wave_and_the_workgroup(ctx, k):
    rng = np.random.default_rng(9300 + k)
    for si, n in enumerate(_sizes(k)):
        if n < k:
            continue
        q = _query(rng, k)
        codes = _text(rng, n, k, q)
        e = ko.ends(codes, k, po.from_2bit(q, k))
        ref = Ref(codes, off=(0, 1, 7, 15)[(si + k) % 4], woff=(si + k // 4) % 2, rng=rng)
        for ti, tau in enumerate(sorted({0, 2, k})):
            want = ho.of_ends(e, tau)
            total = want[0].size
            assert tau < k or total == n
            layout = ("ascii", "packed")[(si + ti) % 2] if n > 2 * C else None  # both layouts at the small sizes, alternating at the large ones
            for lay in (("ascii", "packed") if layout is None else (layout,)):
                got = _hits(ctx, ref, lay, k, q, tau, total + 40)
                _check(got, want, total + 40, (k, n, tau, lay))
                assert _count1(ctx, ref, lay, k, q, tau) == got[0]
                if total:
                    be, bd = _best1(ctx, ref, lay, k, q)
                    assert bd == int(got[2].min()) and be == int(got[1][np.argmin(got[2])])  # min(hit_dist) and its first end: the best match


# ---- 2. cap and the emit pass ---------------------------------------------------------------------------------------------------------------
def test_every_cap_with_and_without_hit_dist(ctx):
    rng = np.random.default_rng(202)
    k, n = 16, WAVE + 1
    q = _query(rng, k)
    codes = _text(rng, n, k, q, copies=24)
    codes[n - k:] = _qcodes(q, k)  # a hit in the last column, the only one of the second wave
    want = ho.hits(codes, k, po.from_2bit(q, k), 2)
    total = want[0].size
    assert total >= 20 and int(want[0][-1]) == n
    ref = Ref(codes, off=1, woff=1, rng=rng)
    sing = po.from_2bit(q, k)
    for cap in (0, 1, total - 1, total, total + 1):
        for with_dist in (True, False):
            for layout in ("ascii", "packed"):
                for pattern in (False, True):
                    got = _hits(ctx, ref, layout, k, sing if pattern else q, 2, cap, pattern, with_dist)
                    _check(got, want, cap, (cap, with_dist, layout, pattern), with_dist)


def test_every_end_a_hit(ctx):
    rng = np.random.default_rng(203)
    k, n = 16, GROUP + 1
    q = _query(rng, k)
    codes = _text(rng, n, k, q)
    e = ko.ends(codes, k, po.from_2bit(q, k))
    ref = Ref(codes, off=7, woff=1, rng=rng)
    for layout, tau in (("ascii", k), ("packed", 2**32 - 1)):
        total, end, dist = _hits(ctx, ref, layout, k, q, tau, n + 5)
        assert total == n and np.array_equal(end, np.arange(1, n + 1, dtype=np.uint64)) and np.array_equal(dist, e.astype(np.uint8))
    total, end, dist = _hits(ctx, ref, "ascii", k, q, k, n - 3 * C - 7)  # cap inside a chunk in the middle of a wave
    assert total == n and np.array_equal(end, np.arange(1, n - 3 * C - 7 + 1, dtype=np.uint64))


# ---- 3. the seams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [C, WAVE, GROUP], ids=["chunk", "wave", "workgroup"])
@pytest.mark.parametrize("k,d", [(16, 1), (16, 4), (31, 7)])
def test_a_planted_bulge_behind_the_seam(ctx, k, d, seam):
    """a copy of the query with d inserted bases that ends e = 1 .. 2k + 1 columns behind the seam: the lane behind the seam needs its lead-in for it, and
    the lane before the seam, whose columns the lead-in repeats, reports nothing of it twice"""
    n = seam + 2 * k + 300
    for e in range(1, 2 * k + 2):
        rng = np.random.default_rng(seam + 100 * k + e)
        if seam == C:  # a random reference and the DP over all of it
            q = _query(rng, k)
            codes = rng.integers(0, 4, size=n)
            codes[seam + e - (k + d):seam + e] = _with_insert(rng, _qcodes(q, k), d)
            want = ho.hits(codes, k, po.from_2bit(q, k), d)
        else:  # all A and a query without A: the DP around the plant only (sparse_hits)
            qc = rng.integers(1, 4, size=k)
            q = _word(qc)
            plant = _with_insert(rng, qc, d)
            codes = np.zeros(n, dtype=np.int64)
            codes[seam + e - (k + d):seam + e] = plant
            want = ho.sparse_hits(n, [(seam + e - (k + d), plant)], k, po.from_2bit(q, k), d)
        assert (seam + e) in want[0]
        lay = ("ascii", "packed")[e % 2]
        ref = Ref(codes, off=e % 4, woff=e % 2, layouts=(lay,))
        _check(_hits(ctx, ref, lay, k, q, d, want[0].size + 9), want, want[0].size + 9, (k, d, seam, e))


@pytest.mark.parametrize("seam", [C, WAVE, GROUP], ids=["chunk", "wave", "workgroup"])
def test_exact_copies_on_both_sides_of_the_seam(ctx, seam):
    rng = np.random.default_rng(seam + 19)
    k = 16
    n = seam + C + 300
    for e in (1, 2, k, 2 * k - 1, 2 * k, 2 * k + 1):
        q = _query(rng, k)
        codes = rng.integers(0, 4, size=n)
        codes[seam + e - k:seam + e] = _qcodes(q, k)  # ends e columns behind the seam
        codes[seam - 40:seam - 40 + k] = _qcodes(q, k)  # ends at seam - 24: a column of the lead-in of the seam's chunk, which the chunk before reports
        codes[seam - k:seam] = _qcodes(q, k) if e > k else codes[seam - k:seam]  # and one that ends in the last column before the seam
        for tau in (0, 1):
            want = ho.hits(codes, k, po.from_2bit(q, k), tau)
            assert {seam + e, seam - 24}.issubset(set(want[0].tolist())) and (e <= k or seam in want[0])
            assert tau == 0 or {seam + e - 1, seam + e + 1}.issubset(set(want[0].tolist()))  # the run around an exact copy
            _both(ctx, codes, k, q, tau, (seam, e, tau), off=e % 4, woff=e % 2, want=want)


# ---- 4. chunks without hits -------------------------------------------------------------------------------------------------------------------
def _a_reference(n, k, q, plants):
    """all A with exact copies of q at the 0-based starts `plants`"""
    codes = np.zeros(n, dtype=np.int64)
    for p in plants:
        codes[p:p + k] = _qcodes(q, k)
    return codes


def test_hits_in_a_few_chunks_only(ctx):
    """hits in chunks 0, 63, 64 and the last of 3 waves + a bit: waves with a single non-empty lane, and one with none"""
    k = 20
    q = _word([1, 2, 3] * 6 + [1, 2])  # no A: the background is at distance k
    n = 3 * WAVE + 5 * C + 77
    last = (n - 1) // C
    codes = _a_reference(n, k, q, [100, 63 * C + 500, 64 * C + 3, last * C + 10])
    want = ho.hits(codes, k, po.from_2bit(q, k), 1)
    assert sorted(set(((want[0] - 1) // C).tolist())) == [0, 63, 64, last] and want[0].size == 12
    _both(ctx, codes, k, q, 1, "sparse chunks", off=1, woff=1, want=want)
    want = ho.hits(codes, k, po.from_2bit(q, k), 0)
    assert want[0].size == 4
    _both(ctx, codes, k, q, 0, "sparse chunks, tau 0", off=7, want=want, slack=0)


def test_every_second_chunk_empty(ctx):
    k = 20
    q = _word([1, 2, 3] * 6 + [1, 2])
    n = 70 * C + 11
    codes = _a_reference(n, k, q, [c * C + (37 * c) % (C - 2 * k) + k for c in range(0, 70, 2)])
    want = ho.hits(codes, k, po.from_2bit(q, k), 2)
    assert sorted(set(((want[0] - 1) // C).tolist())) == list(range(0, 70, 2))
    _both(ctx, codes, k, q, 2, "every second chunk", off=15, woff=1, want=want)


# ---- 5. the scan's tile seam, in chunk units ------------------------------------------------------------------------------------------------
def test_hits_around_the_scan_tile_seam(ctx):
    """4097 C + 5 ends are 4098 entries of the scan: two tiles.  Plants in chunks 4094 .. 4097 (two per chunk, so that an offset that loses the
    first tile's total, or a chunk's count, shows) and a few in the first tile"""
    k = 24
    qc = [1, 2, 3, 3, 2, 1] * 4
    q = _word(qc)
    n = (TILE + 1) * C + 5
    plants = [(500, np.array(qc)), (7 * C + 9, np.insert(np.array(qc), 11, 2))]
    for c in range(TILE - 2, TILE + 1):
        plants.append((c * C + 100, np.array(qc)))
        plants.append((c * C + 700, np.delete(np.array(qc), 5)))
    plants.append((n - k + 1, np.delete(np.array(qc), 5)))  # chunk 4097 has five columns: this plant ends in the last one
    sing = po.from_2bit(q, k)
    want = ho.sparse_hits(n, plants, k, sing, 1)
    assert want[0].size >= 15 and int(want[0][-1]) == n and {TILE - 2, TILE - 1, TILE, TILE + 1}.issubset(set(((want[0] - 1) // C).tolist()))
    codes = np.zeros(n, dtype=np.int64)
    for p, c in plants:
        codes[p:p + len(c)] = c
    _both(ctx, codes, k, q, 1, "tile seam", off=1, woff=1, want=want, slack=3)
    ref = Ref(codes, layouts=("packed",))
    cap = want[0].size - 5  # cap reached inside the second tile
    _check(_hits(ctx, ref, "packed", k, sing, 1, cap, pattern=True), want, cap, "tile seam, capped")


# ---- 6. lead and pos_base: the host forms above the host cutoff -----------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context():
    import bitnuc_amd as bn
    rng = np.random.default_rng(811)
    n, k = 1_500_000, 23
    q = _query(rng, k)
    codes = _text(rng, n, k, q, copies=12)
    s = _ascii(codes, rng)
    w = po.pack_codes(codes, junk=2**64 - 1)
    sing = po.from_2bit(q, k)
    c = bn.Context(0)
    try:
        assert n >= 1 << 20
        for tau in (0, 3):
            want = ho.hits(codes, k, sing, tau)
            assert want[0].size >= 3
            for got in (c.kmer_edist_hits(s, k, q, tau, with_dist=True), c.kmer_edist_hits_packed(w, n, k, q, tau, with_dist=True),
                        c.kmer_pattern_edist_hits(s, k, sing, tau, with_dist=True), c.kmer_pattern_edist_hits_packed(w, n, k, sing, tau, with_dist=True)):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(c.kmer_edist_hits(s, k, q, tau), want[0])  # hit_dist NULL
        b = s.copy()
        b[n - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.kmer_edist_hits(b, k, q, 1)
        assert (ei.value.byte, ei.value.index) == (ord("N"), n - 5)
        del ei
        assert np.array_equal(c.kmer_edist_hits(s, k, q, 3), want[0])  # the next call is clean
    finally:
        c.close()


def _raw_host_hits(ctx, fn, head, k, q, tau, cap):
    """the raw host entry point on the live context with a caller's cap: (total, end, dist), guard words checked"""
    from bitnuc_amd import _lib as L
    end = np.full(cap + 4, FILL, dtype=np.uint64)
    dist = np.full(cap + 4, 0x5A, dtype=np.uint8)
    total = C_.c_uint64(0)
    err = L.BitnucErr()
    st = fn(ctx._h, *head, k, q, tau, C_.c_void_p(end.ctypes.data), C_.c_void_p(dist.ctypes.data), cap, C_.byref(total), C_.byref(err))
    assert st == L.OK
    m = min(cap, total.value)
    assert (end[m:] == np.uint64(FILL)).all() and (dist[m:] == 0x5A).all(), "written at or beyond min(cap, total)"
    return total.value, end[:m], dist[:m]


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff run in chunks of 128 Mi ends, each behind the 2k bases before it (packed: whole words), which are run but not
    reported; the chunk's ends come back shifted by its first column.  An all-A reference of 128 Mi + 3 M bases with planted copies of a query without A
    (expected values: kmer_edist_hits_oracle.sparse_hits): a copy with one inserted base ACROSS the boundary (its last base 9 behind it: chunk 1 needs
    its lead-in), an exact copy that ends 30 bases before the boundary (inside chunk 1's lead-in: chunk 0 reports it, once), copies in both chunks.
    Then cap reached inside the first chunk, and cap spanning the boundary."""
    rng = np.random.default_rng(1283)
    chunk = 128 << 20
    n, k = chunk + 3_000_000, 25
    qc = rng.integers(1, 4, size=k)  # no A: the background is at distance k
    bulge = np.insert(qc, 12, 2)
    near = qc.copy()
    near[7] = near[7] % 3 + 1
    plants = [(5_000_000, near), (chunk - 30 - k, qc), (chunk + 9 - len(bulge), bulge), (chunk + 1_000_000, near), (chunk + 2_000_000, qc)]
    q = _word(qc) | (0xABC << (2 * k))  # junk above 2k
    sing = po.from_2bit(q, k)
    want = ho.sparse_hits(n, plants, k, sing, 1)
    assert {5_000_000 + k, chunk - 30, chunk + 9, chunk + 1_000_000 + k, chunk + 2_000_000 + k}.issubset(set(want[0].tolist()))
    in_first = int((want[0] <= chunk).sum())
    assert 4 <= in_first < want[0].size - 4
    codes = np.zeros(n, dtype=np.uint8)
    for p, c in plants:
        codes[p:p + len(c)] = c
    s = LUT[codes]
    del codes
    got = ctx.kmer_edist_hits(s, k, q, 1, with_dist=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    sp = C_.c_void_p(s.ctypes.data)
    for cap in (2, in_first + 2):  # reached inside the first chunk; spanning the boundary
        got = _raw_host_hits(ctx, ctx._lib.bitnuc_kmer_edist_hits, (sp, n), k, C_.c_uint64(q), 1, cap)
        assert got[0] == want[0].size and np.array_equal(got[1], want[0][:cap]) and np.array_equal(got[2], want[1][:cap]), cap
    w = oracle.encode(s)
    got = ctx.kmer_pattern_edist_hits_packed(w, n, k, sing, 1, with_dist=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = _raw_host_hits(ctx, ctx._lib.bitnuc_kmer_edist_hits_packed, (C_.c_void_p(w.ctypes.data), w.size, n), k, C_.c_uint64(q), 1, in_first + 1)
    assert got[0] == want[0].size and np.array_equal(got[1], want[0][:in_first + 1]) and np.array_equal(got[2], want[1][:in_first + 1])


# ---- 7. past 2^32 bases and past the grid's round ---------------------------------------------------------------------------------------------
def test_packed_reference_past_32_bits(ctx):
    """2^32 + 70,000 bases of A as zero words: copies of the query with inserted bases that end 2k before and 2k behind base 2^29 (a round of the
    bounded grid covers at most 2^29 bases), one just past base 2^32 and an exact copy near the end; the expected values come from the oracle on each
    plant's neighbourhood (kmer_edist_hits_oracle.sparse_hits).  Ends above 2^32 in end[], more than 4 M entries and 1024 tiles in the scan."""
    import torch
    dev = torch.device("cuda:0")
    n, k = (1 << 32) + 70_000, 31
    rng = np.random.default_rng(3233)
    qc = rng.integers(1, 4, size=k)
    bulge = np.insert(np.insert(qc, 20, 1), 9, 3)
    one = np.insert(qc, 15, 2)
    plants = [(1000, qc), ((1 << 29) - 2 * k - len(one), one), ((1 << 29) + 2 * k - len(bulge), bulge), (3 * (1 << 29) - 10, one), ((1 << 32) + 40, bulge),
              (n - 1000, qc)]
    q = _word(qc)
    want = ho.sparse_hits(n, plants, k, po.from_2bit(q, k), 2)
    assert {(1 << 29) - 2 * k, (1 << 29) + 2 * k, (1 << 32) + 40 + k + 2, n - 1000 + k}.issubset(set(want[0].tolist())) and want[0].size >= 12
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
    cap = want[0].size + 6
    o = Out(cap)
    torch.cuda.synchronize()
    ctx.kmer_edist_hits_packed_async(words, nw, n, k, q, 2, *o.args())
    _check(o.read(ctx), want, cap, "past 2^32")
    o = Out(want[0].size - 2)  # cap reached past 2^32
    ctx.kmer_edist_hits_packed_async(words, nw, n, k, q, 2, *o.args())
    _check(o.read(ctx), want, want[0].size - 2, "past 2^32, capped")


# ---- 8. invalid bytes -------------------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_latched_once_with_the_smallest_index(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(56)
    k = 16
    n = 3 * C + 77
    q = _query(rng, k)
    codes = _text(rng, n, k, q)
    s = _ascii(codes, rng)
    for case, at in enumerate(((0,), (n - 1,), (C - 10,), (2 * C - 64,), (2 * C + 5, C + 3), (n - 1, 2 * C - 1))):  # C - 10, 2C - 64: in a chunk's lead-in
        b = s.copy()
        for i, a in enumerate(at):
            b[a] = (ord("N"), ord("x"))[i]
        first = min(at)
        for cap in (0, 64):  # with and without the emit pass, which latches nothing
            t, ptr = _ascii_dev(b, (0, 1, 7, 15)[case % 4])
            o = Out(cap)
            torch.cuda.synchronize()
            ctx.kmer_edist_hits_async(ptr, n, k, q, k, *o.args())
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (int(b[first]), first), (case, cap)
            del ei
            ctx.sync()  # latched once: nothing left for the next sync
    _both(ctx, codes, k, q, 2, "clean after the errors", rng=rng)


# ---- 9. patterns --------------------------------------------------------------------------------------------------------------------------------
def test_patterns_singletons_a_guide_with_ngg_and_a_barcode_with_ns(ctx):
    rng = np.random.default_rng(909)
    n = 5 * C + 123
    # singletons: the exact form's outputs, all of them
    k = 17
    q = _query(rng, k)
    codes = _text(rng, n, k, q, copies=8)
    ref = Ref(codes, off=7, woff=1, rng=rng)
    for tau in (0, 2):
        for layout in ("ascii", "packed"):
            a = _hits(ctx, ref, layout, k, q, tau, n)
            b = _hits(ctx, ref, layout, k, po.from_2bit(q, k), tau, n, pattern=True)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[0] >= 1
    # the four asynchronous methods by name, cap cutting the list
    want = ho.hits(codes, k, po.from_2bit(q, k), 2)
    outs = [Out(want[0].size - 1) for _ in range(4)]
    ctx.kmer_edist_hits_async(*ref.heads["ascii"], k, q, 2, *outs[0].args())
    ctx.kmer_edist_hits_packed_async(*ref.heads["packed"], k, q, 2, *outs[1].args())
    ctx.kmer_pattern_edist_hits_async(*ref.heads["ascii"], k, po.from_2bit(q, k), 2, *outs[2].args())
    ctx.kmer_pattern_edist_hits_packed_async(*ref.heads["packed"], k, po.from_2bit(q, k), 2, *outs[3].args())
    for o in outs:
        _check(o.read(ctx), want, want[0].size - 1, "by name")
    # a 20-base guide + NGG (k = 23) with a bulge in one copy, and a barcode with Ns
    guide = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=20))
    for pat, k in ((guide + "NGG", 23), ("ACNNGTTNCAGGNT", 14)):
        p = po.from_iupac(pat)
        codes = rng.integers(0, 4, size=n)
        concrete = np.array([("ACGT".index(ch) if ch in "ACGT" else int(rng.integers(0, 4))) for ch in pat])
        codes[C - 5:C - 5 + k] = concrete  # an exact occurrence across a chunk seam
        codes[3 * C + 50:3 * C + 50 + k + 1] = np.insert(concrete, 9, 0)  # one with a bulge
        codes[4 * C + 700:4 * C + 700 + k - 1] = np.delete(concrete, 4)
        for tau in (0, 1, 2):
            want = ho.hits(codes, k, p, tau)
            assert (C - 5 + k) in want[0] and (tau == 0 or (3 * C + 50 + k + 1) in want[0])
            _both(ctx, codes, k, None, tau, (pat, tau), off=1, woff=1, rng=rng, pattern=p, want=want)


# ---- 11. a hipGraph replay ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reference_and_the_outputs_changed():
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(79)
    n, k = 70_001, 23
    q = _query(rng, k)
    c1, c2 = _text(rng, n, k, q, copies=6), _text(rng, n, k, q, copies=10)
    sing = po.from_2bit(q, k)
    want1, want2 = ho.hits(c1, k, sing, 2), ho.hits(c2, k, sing, 2)
    assert not np.array_equal(want1[0], want2[0]) and want1[0].size >= 3 and want2[0].size >= 3
    cap = max(want1[0].size, want2[0].size) - 1  # the same cap in both: the second list is cut
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(_ascii(c1), 7)
        w = po.pack_codes(c1)
        tw, wptr = _words_dev(w, 1)
        oa, op = Out(cap), Out(cap)

        def enqueue():
            c.kmer_edist_hits_async(ptr, n, k, q, 2, *oa.args())
            c.kmer_pattern_edist_hits_packed_async(wptr, w.size, n, k, sing, 2, *op.args())

        enqueue()  # warm-up outside the capture: sizes the scratch
        _check(oa.read(c), want1, cap, "warm-up ascii")
        _check(op.read(c), want1, cap, "warm-up packed")
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                enqueue()
            t[7:7 + n] = torch.from_numpy(_ascii(c2)).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(po.pack_codes(c2).view(np.int64)).to(tw.device)
            for _ in range(2):
                oa.refill()
                op.refill()
                g.replay()
                _check(oa.read(c), want2, cap, "replay ascii")
                _check(op.read(c), want2, cap, "replay packed")
        finally:
            g.reset()
            del g
            c.close()


# ---- 12. a queue with one sync ----------------------------------------------------------------------------------------------------------------
def test_mixed_queue_with_hamming_hit_lists_and_one_sync(ctx, oracle):
    """Hamming hits -> edit hits -> edit best -> Hamming hits -> edit count on one context, several rounds with different sizes, one sync at the end:
    the hit lists share context scratch 7, the edit best match and count scratch 9, in stream order"""
    import torch
    rng = np.random.default_rng(608)
    k = 21
    dev = torch.device("cuda:0")
    jobs = []
    for i, n in enumerate((30_001, 5 * C + 3, 70_000, 2 * C)):
        q = _query(rng, k) & (2**64 - 1)
        codes = _text(rng, n, k, q, copies=8)
        s = _ascii(codes, rng)
        w = po.pack_codes(codes)
        jobs.append(dict(i=i, n=n, q=q, codes=codes, s=s, w=w, ascii=_ascii_dev(s, (0, 7, 1, 15)[i]), wdev=_words_dev(w, i & 1),
                         dq=_dev(np.array([q], dtype=np.uint64), np.int64), dt=_dev(np.array([3], dtype=np.uint32), np.int32),
                         h1=Out(n), e=Out(n), h2=Out(n), be=torch.zeros(1, dtype=torch.int64, device=dev), bd=torch.zeros(1, dtype=torch.uint8, device=dev),
                         cnt=torch.zeros(1, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        n, q, ptr, wp, nw = j["n"], j["q"], j["ascii"][1], j["wdev"][1], j["w"].size
        ctx.kmer_hdist_hits_dev(ptr, n, k, q, 3, *j["h1"].args())
        if j["i"] % 2 == 0:
            ctx.kmer_edist_hits_async(ptr, n, k, q, 3, *j["e"].args())
        else:
            ctx.kmer_edist_hits_packed_async(wp, nw, n, k, q, 3, *j["e"].args())
        ctx.kmer_edist_best_async(ptr, n, k, j["dq"], 1, j["be"], j["bd"])
        ctx.kmer_hdist_hits_packed_dev(wp, nw, n, k, q, 2, *j["h2"].args())
        ctx.kmer_edist_count_multi_packed_async(wp, nw, n, k, j["dq"], j["dt"], 1, j["cnt"])
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        n, q = j["n"], j["q"]
        e = ko.ends(j["codes"], k, po.from_2bit(q, k))
        want = ho.of_ends(e, 3)
        _check(j["e"].read(ctx), want, n, ("queue", j["i"]))
        assert int(j["cnt"].cpu().numpy().view(np.uint64)[0]) == want[0].size
        assert (int(j["be"].cpu().numpy().view(np.uint64)[0]), int(j["bd"].cpu()[0])) == (int(np.argmin(e)) + 1, int(e.min()))
        d = oracle.kmer_hdist_scan(j["s"], k, int(q))
        for out, tau in ((j["h1"], 3), (j["h2"], 2)):
            total, pos, hd = out.read(ctx)
            at = np.nonzero(d <= tau)[0]
            assert total == at.size and np.array_equal(pos, at.astype(np.uint64)) and np.array_equal(hd, d[at].astype(np.uint8))


# ---- 13. a seeded fuzz ------------------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz(ctx):
    """200 cases with n <= 3 C: a random reference with a copy of the query that carries 1 .. tau inserted or deleted bases (an indel hit: within tau by
    edit distance, beyond tau by Hamming distance at the same end) and at least one chunk without a hit -- both asserted of every generated case"""
    rng = np.random.default_rng(0xF022)
    cases = 0
    draws = 0
    while cases < 200:
        draws += 1
        assert draws < 400, "the generator does not produce the cases it promises"
        k = int(rng.integers(12, 33))
        tau = int(rng.integers(1, 4))
        n = int(rng.integers(C + 1, 3 * C + 1))
        q = _query(rng, k)
        qc = _qcodes(q, k)
        codes = rng.integers(0, 4, size=n)
        d = int(rng.integers(1, tau + 1))
        c = qc.copy()
        for _ in range(d):
            at = int(rng.integers(1, len(c) - 1))
            c = np.insert(c, at, int(rng.integers(0, 4))) if rng.integers(0, 2) else np.delete(c, at)
        p = int(rng.integers(0, n - len(c) + 1))
        codes[p:p + len(c)] = c
        if rng.integers(0, 3) == 0:  # and sometimes an exact copy as well
            p2 = int(rng.integers(0, n - k + 1))
            if p2 + k <= p or p2 >= p + len(c):
                codes[p2:p2 + k] = qc
        sing = po.from_2bit(q, k)
        want = ho.hits(codes, k, sing, tau)
        end = p + len(c)
        indel = end in want[0] and end >= k and int((codes[end - k:end] != qc).sum()) > tau
        nchunks = (n + C - 1) // C
        empty = len(set(((want[0] - 1) // C).tolist())) < nchunks
        if not (indel and empty):
            continue
        cases += 1
        layout = ("ascii", "packed")[cases % 2]
        ref = Ref(codes, off=(0, 1, 7, 15)[cases % 4], woff=(cases // 2) % 2, rng=rng, layouts=(layout,))
        cap = (want[0].size + 3, want[0].size, max(want[0].size - 1, 0))[cases % 3]
        pattern = cases % 5 == 0
        _check(_hits(ctx, ref, layout, k, sing if pattern else q, tau, cap, pattern), want, cap, ("fuzz", cases, k, tau, n, layout))


# ---- 14. the C++ mirror -------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_of_the_kmer_edist_hits_forms(ctx, tmp_path):
    """the four kmer_*edist_hits* methods of include/bitnuc.hpp against the plain DP, via tests/cpp/test_kmer_edist_hits_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kmer_edist_hits_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_kmer_edist_hits_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "kmer edist hits hpp ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
