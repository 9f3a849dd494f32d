"""GPU tests of the pattern queries (bitnuc_kmer_pattern_count_multi / _best / _hits [_packed] _async and the host forms above the cutoff): a set of
bases per position, pdist(j) = #{i < k : ref[j+i] not in S_i}, against the numpy brute force of tests/pattern_oracle.py.  Exact integer equality.

Sizes come from the kernels' own constants, read from the headers: no window beyond k, the largest size without a round, the first with one, one whole
trip, a trip + a round + 7, two workgroups and a round.  ASCII references at byte offsets 0 / 1 / 7 / 15, packed words at 0 and 8 mod 16 with n no
multiple of 32; k in {1, 20, 23, 31, 32}; 1 / 16 / 17 / 33 patterns; thresholds 0 / 3 / k - 1 / k / 2^32 - 1 mixed per pattern.  Patterns: singletons,
all-N, exact + NGG, exact + NRG, random sets with empty ones, {T}, {A, T}, all-empty.  Occurrences are planted at window 0, skip - 1, skip, both sides of
a round and of a trip boundary, the last covered window, the first tail window and the last window, so that no case is all-miss and the best match has
ties to resolve.  Every result equals the oracle; singleton patterns equal the exact entry point called beside them; ASCII and packed agree; nothing is
written past n_queries or past cap."""
import os
import re

import numpy as np
import pytest

import pattern_oracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnuc_amd", "csrc")
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = (1, 20, 23, 31, 32)
QS = (1, 16, 17, 33)
ASCII_OFFS = (0, 1, 7, 15)


def _const(fname, name):
    m = re.search(r"constexpr\s+(?:unsigned\s+)?(?:int|unsigned|size_t)\s+" + name + r"\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


MULTI_ROUNDS = _const("scan_multi_device.h", "kMultiRounds")
MULTI_BLOCK = _const("scan_multi_device.h", "kMultiBlock")
MULTI_QB = _const("scan_multi_device.h", "kMultiQB")
HITS_ROUNDS = _const("scan_hits_device.h", "kHitsRounds")
assert MULTI_ROUNDS == HITS_ROUNDS == 4 and MULTI_QB == 16 and set(QS) == {1, MULTI_QB, MULTI_QB + 1, 2 * MULTI_QB + 1}
assert "return nr >= 1056 ? (nr - 32) >> 10 : 0;" in open(os.path.join(CSRC, "scan_mfma_host.h")).read()
WG_ROUNDS = (MULTI_BLOCK // 64) * MULTI_ROUNDS  # rounds one workgroup takes per pass over its waves


def scan_rounds(n, skip):
    nr = n - skip if n > skip else 0
    return (nr - 32) >> 10 if nr >= 1056 else 0


def sizes(k, skip):
    """the six sizes for a reference whose rounds start at base `skip`"""
    trip = 1024 * MULTI_ROUNDS
    out = [k, 1055 + skip, 1056 + skip, skip + trip + 32, skip + trip + 1024 + 32 + 7, skip + (2 * WG_ROUNDS + 1) * 1024 + 32 + 13]
    assert [scan_rounds(n, skip) for n in out[1:]] == [0, 1, MULTI_ROUNDS, MULTI_ROUNDS + 1, 2 * WG_ROUNDS + 1] and 90_000 < out[-1] < 110_000
    return out


def plant_places(n, k, skip):
    """window 0, skip - 1, skip, both sides of a round and of a trip boundary, the last covered window, the first tail window, the last window"""
    nwin, rounds = n - k + 1, scan_rounds(n, skip)
    trip = 1024 * MULTI_ROUNDS
    want = [0, skip - 1, skip, skip + 1023, skip + 1024, skip + trip - 1, skip + trip, skip + 1024 * rounds - 1, skip + 1024 * rounds, nwin - 1]
    return sorted({p for p in want if 0 <= p < nwin})


def make_patterns(rng, k, nq, lead):
    """(patterns, the exact queries of the singletons among them as {index: query}); `lead` rotates which kind comes first.  The first pattern has no
    empty set: an occurrence of it can be planted"""
    pats, singles = [], {}
    for i in range(nq):
        kind = (i + lead) % 8
        if (i == 0 and kind in (4, 7)) or (kind in (2, 3) and k < 4):  # (no room for a PAM below k = 4)
            kind = 6
        exact = [{int(c)} for c in rng.integers(0, 4, size=k)]
        if kind in (0, 5):
            q = sum(next(iter(s)) << (2 * b) for b, s in enumerate(exact))
            singles[i] = q | ((int(rng.integers(1, 2**20)) << (2 * k)) & (2**64 - 1)) if k < 32 else q  # junk above 2k for the exact twin
            pats.append(po.from_sets(exact))
        elif kind == 1:
            pats.append(po.from_iupac("N" * k))
        elif kind in (2, 3):  # k - 3 exact positions + NGG / NRG (k = 23: the guide search)
            pats.append(po.from_sets(exact[:k - 3] + [{0, 1, 2, 3}, {2} if kind == 2 else {0, 2}, {2}]))
        elif kind == 4:
            pats.append(po.from_sets(po.random_sets(rng, k)))
        elif kind == 6:
            pats.append(po.from_sets([{3} if rng.integers(0, 2) else {0, 3} for _ in range(k)]))
        else:
            pats.append(po.from_sets([set()] * k) if i % 3 == 0 else po.from_sets(po.random_sets(rng, k)))
    return pats, singles


def make_taus(k, nq, lead):
    cyc = (0, 3, k - 1, k, 2**32 - 1)
    return np.array([cyc[(i + lead) % 5] for i in range(nq)], dtype=np.uint32)


def make_codes(rng, n, k, skip, pats):
    """random bases with an occurrence of one of the first patterns planted at every place (a base of the set where it is not empty), in ascending
    order; the last place gets the first pattern, so that one occurrence of it is never overwritten by a neighbour"""
    codes = rng.integers(0, 4, size=n)
    places = plant_places(n, k, skip)
    for j, p in enumerate(places):
        pat = pats[0] if p == places[-1] else pats[j % min(len(pats), 3)]
        for i in range(k):
            allowed = [c for c in range(4) if (int(pat[c]) >> i) & 1]
            if allowed:
                codes[p + i] = allowed[int(rng.integers(0, len(allowed)))]
    return codes


def ascii_of(rng, codes):
    s = LUT[codes].copy()
    s[rng.random(codes.size) < 0.3] |= 0x20
    return s


class Want:
    """the oracle's answers for (codes, patterns, taus), computed once and shared by the calls of a case"""

    def __init__(self, codes, k, pats, taus):
        self.d = [po.pdist(codes, p, k) for p in pats]
        self.counts = np.array([po.count(d, int(t)) for d, t in zip(self.d, taus)], dtype=np.uint64)
        b = [po.best(d) for d in self.d]
        self.pos = np.array([x[0] for x in b], dtype=np.uint64)
        self.dist = np.array([x[1] for x in b], dtype=np.uint8)


# ---- device buffers -------------------------------------------------------------------------------------------------------------------------
def _ascii_dev(s, off):
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    t[off:off + s.size] = torch.from_numpy(s)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _words_dev(w, off):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    assert (t.data_ptr() + 8 * off) % 16 == 8 * off
    return t, t.data_ptr() + 8 * off


def _patterns_dev(pats, dword_off):
    """the patterns in device memory at 4 * dword_off bytes past an aligned address: 4-byte alignment is all they need"""
    import torch
    flat = np.ascontiguousarray(np.stack(pats)).reshape(-1).view(np.int32)
    t = torch.zeros(flat.size + dword_off, dtype=torch.int32, device="cuda:0")
    t[dword_off:] = torch.from_numpy(flat.copy())
    return t, t.data_ptr() + 4 * dword_off


def _u64_dev(a):
    import torch
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _u32_dev(a):
    import torch
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def _guarded64(n):
    import torch
    return torch.full((n + GUARD,), FILL, dtype=torch.int64, device="cuda:0")


def _guarded8(n, off=1):
    import torch
    t = torch.full((off + n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    return t, t.data_ptr() + off


def _read64(t, n, what):
    a = t.cpu().numpy().view(np.uint64)
    assert (a[n:] == np.uint64(FILL)).all(), what + ": written past its end"
    return a[:n].copy()


def _read8(t, n, what, off=1):
    a = t.cpu().numpy()
    assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), what + ": written outside its range"
    return a[off:off + n].copy()


class Dev:
    """one reference on the device, as ASCII at a byte offset or as packed words at a word offset"""

    def __init__(self, ctx, codes, s, packed, off):
        self.ctx, self.packed, self.n = ctx, packed, codes.size
        if packed:
            self.w = po.pack_codes(codes, junk=0xDEADBEEFCAFEF00D)
            self.keep, self.ptr = _words_dev(self.w, off)
        else:
            self.keep, self.ptr = _ascii_dev(s, off)

    def head(self):
        return (self.ptr, self.w.size, self.n) if self.packed else (self.ptr, self.n)

    def count(self, k, dq, dt, nq, pattern=True):
        import torch
        out = _guarded64(nq)
        torch.cuda.synchronize()
        name = ("kmer_pattern_count_multi" if pattern else "kmer_hdist_count_multi") + ("_packed" if self.packed else "") + ("_async" if pattern else "_dev")
        getattr(self.ctx, name)(*self.head(), k, dq, dt, nq, out)
        self.ctx.sync()
        return _read64(out, nq, name)

    def best(self, k, dq, nq, pattern=True):
        import torch
        pos = _guarded64(nq)
        dbuf, dptr = _guarded8(nq)
        torch.cuda.synchronize()
        name = ("kmer_pattern_best" if pattern else "kmer_hdist_best") + ("_packed" if self.packed else "") + "_async"
        getattr(self.ctx, name)(*self.head(), k, dq, nq, pos, dptr)
        self.ctx.sync()
        return _read64(pos, nq, name), _read8(dbuf, nq, name)

    def hits(self, k, query, tau, cap, with_dist, pattern=True):
        """(positions, distances or None, total); query: a (4,) pattern or an exact query"""
        import torch
        pos = _guarded64(cap)
        dbuf, dptr = _guarded8(cap)
        nh = _guarded64(1)
        torch.cuda.synchronize()
        name = ("kmer_pattern_hits" if pattern else "kmer_hdist_hits") + ("_packed" if self.packed else "") + ("_async" if pattern else "_dev")
        getattr(self.ctx, name)(*self.head(), k, query, int(tau), pos if cap else None, dptr if with_dist else None, cap, nh)
        self.ctx.sync()
        total = int(_read64(nh, 1, name)[0])
        kept = min(cap, total)
        d = _read8(dbuf, cap, name)
        if not with_dist:
            assert (d == 0x5A).all(), "distances written without being asked for"
        return _read64(pos, cap, name)[:kept], (d[:kept] if with_dist else None), total


def _check_case(ctx, k, codes, s, pats, singles, taus, packed, off, pat_off):
    nq = len(pats)
    want = Want(codes, k, pats, taus)
    dev = Dev(ctx, codes, s, packed, off)
    keep_p, dp = _patterns_dev(pats, pat_off)
    dt = _u32_dev(taus)
    tag = (k, codes.size, nq, packed, off)
    counts = dev.count(k, dp, dt, nq)
    assert np.array_equal(counts, want.counts), (tag, np.nonzero(counts != want.counts)[0][:5], counts[:5], want.counts[:5])
    assert counts[0] > 0 and want.dist[0] == 0  # the planted occurrence of the first pattern: not an all-miss case
    pos, dist = dev.best(k, dp, nq)
    assert np.array_equal(dist, want.dist) and np.array_equal(pos, want.pos), (tag, np.nonzero((pos != want.pos) | (dist != want.dist))[0][:5])
    if singles:  # the singleton patterns against the exact entry points, called beside them
        idx = sorted(singles)
        dq = _u64_dev([singles[i] for i in idx])
        ecounts = dev.count(k, dq, _u32_dev(taus[idx]), len(idx), pattern=False)
        epos, edist = dev.best(k, dq, len(idx), pattern=False)
        assert np.array_equal(ecounts, counts[idx]) and np.array_equal(epos, pos[idx]) and np.array_equal(edist, dist[idx]), tag
    for i in range(min(nq, 3)):  # hit lists: the first patterns, every cap, with and without distances
        hp, hd, total = po.hits(want.d[i], int(taus[i]), 1 << 40)
        assert total == want.counts[i]
        for cap in sorted({0, max(total - 1, 0), total, total + 5}):
            for with_dist in (True, False):
                gp, gd, gt = dev.hits(k, pats[i], taus[i], cap, with_dist)
                kept = min(cap, total)
                assert gt == total and np.array_equal(gp, hp[:kept]), (tag, i, cap)
                assert not with_dist or np.array_equal(gd, hd[:kept]), (tag, i, cap)
        if i in singles:
            ep, ed, et = dev.hits(k, singles[i], taus[i], total + 5, True, pattern=False)
            assert et == total and np.array_equal(ep, hp) and np.array_equal(ed, hd), tag
    return counts, pos, dist


@pytest.mark.parametrize("si", range(6))
@pytest.mark.parametrize("k", KS)
def test_every_size_offset_query_count_and_threshold(ctx, k, si):
    ki = KS.index(k)
    nq = QS[(si + ki) % 4]
    # two of the four ASCII offsets and both packed alignments per case; over the five k every size meets every offset
    for packed, off in ((False, ASCII_OFFS[(si + ki) % 4]), (False, ASCII_OFFS[(si + ki + 2) % 4]), (True, 0), (True, 1)):
        skip = (32 if off else 0) if packed else (16 - off) % 16
        n = sizes(k, skip)[si]
        if packed and n % 32 == 0 and n > k:
            n += 1  # packed: n is no multiple of 32 (the last word carries junk above its bases)
        rng = np.random.default_rng(77_000 + 1000 * k + 10 * si + off + 5 * packed)
        pats, singles = make_patterns(rng, k, nq, lead=si + ki)
        taus = make_taus(k, nq, lead=si)
        codes = make_codes(rng, n, k, skip, pats)  # the places follow the layout's skip
        _check_case(ctx, k, codes, ascii_of(rng, codes), pats, singles, taus, packed, off, pat_off=(si + ki + packed) % 2)


def test_ascii_and_packed_agree_on_the_decoded_words(ctx):
    """one set of bases, as ASCII at +7 and as packed words at 8 mod 16: the same answers from both front ends (and the oracle's)"""
    k, nq = 23, 33
    rng = np.random.default_rng(4242)
    n = sizes(k, 32)[4] + 3
    pats, singles = make_patterns(rng, k, nq, lead=2)
    taus = make_taus(k, nq, lead=1)
    codes = make_codes(rng, n, k, 32, pats)
    s = ascii_of(rng, codes)
    assert np.array_equal(po.codes_of_words(po.pack_codes(codes), n), codes) and np.array_equal(po.codes_of_ascii(s), codes)
    a = _check_case(ctx, k, codes, s, pats, singles, taus, False, 7, 1)
    p = _check_case(ctx, k, codes, s, pats, singles, taus, True, 1, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, p))


def test_best_match_ties_resolve_to_the_leftmost_window(ctx):
    """the PAM pattern planted at every boundary place with distance 0, and once more with one guide mismatch further left: distance 0 wins and, among
    the equal ones, the leftmost; under all-N every window ties at 0 and window 0 wins; under the empty pattern every window ties at k"""
    k, off = 23, 7
    skip = (16 - off) % 16
    rng = np.random.default_rng(31)
    n = sizes(k, skip)[4]
    guide = [{int(c)} for c in rng.integers(0, 4, size=20)]
    pam = po.from_sets(guide + [{0, 1, 2, 3}, {2}, {2}])
    pats = [pam, po.from_iupac("N" * k), po.from_sets([set()] * k)]
    codes = rng.integers(0, 4, size=n)
    site = [next(iter(g)) for g in guide] + [1, 2, 2]
    places = []
    for p in plant_places(n, k, skip):  # those that do not overlap an earlier one
        if p >= 100 and (not places or p >= places[-1] + k):
            places.append(p)
    for p in places:
        codes[p:p + k] = site
    codes[40:40 + k] = site
    codes[40 + 5] ^= 1  # further left, one mismatch
    d = po.pdist(codes, pam, k)
    first = int(np.argmin(d))
    assert d[40] == 1 and first == places[0] and len(places) >= 3 and all(d[p] == 0 for p in places)
    s = ascii_of(rng, codes)
    # ASCII at +7, then packed words at 8 mod 16 (their rounds start at base 32: other windows sit at the boundaries, the answer is the same)
    for packed, o, pat_off in ((False, off, 1), (True, 1, 0)):
        dev = Dev(ctx, codes, s, packed, o)
        keep, dp = _patterns_dev(pats, pat_off)
        pos, dist = dev.best(k, dp, 3)
        assert list(pos) == [first, 0, 0] and list(dist) == [0, 0, k], (packed, pos, dist)


def test_invalid_reference_byte_is_reported_by_the_sync_with_the_first_index(ctx):
    """N is a pattern letter and still no reference base: a data error latched on the device, reported once, the next call clean"""
    import torch
    import bitnuc_amd as bn
    k, nq, n = 23, 17, 30_000
    rng = np.random.default_rng(5)
    pats, _ = make_patterns(rng, k, nq, lead=1)
    taus = make_taus(k, nq, lead=0)
    codes = rng.integers(0, 4, size=n)
    s = ascii_of(rng, codes)
    keep, dp = _patterns_dev(pats, 1)
    dt = _u32_dev(taus)
    for bad_at, off in ((17_337, 0), (n - 3, 5), (2, 9)):  # a middle round, the tail, the head
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        out, pos, nh = _guarded64(nq), _guarded64(nq), _guarded64(1)
        dbuf, dptr = _guarded8(nq)
        for call in (lambda: ctx.kmer_pattern_count_multi_async(ptr, n, k, dp, dt, nq, out), lambda: ctx.kmer_pattern_best_async(ptr, n, k, dp, nq, pos, dptr),
                     lambda: ctx.kmer_pattern_hits_async(ptr, n, k, pats[0], 3, None, None, 0, nh)):
            torch.cuda.synchronize()
            call()
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
            del ei
            ctx.sync()  # latched once: nothing left for the next sync
    want = Want(codes, k, pats, taus)
    dev = Dev(ctx, codes, s, False, 3)
    assert np.array_equal(dev.count(k, dp, dt, nq), want.counts)


def test_graph_capture_and_two_replays_of_the_pattern_count():
    import torch
    import bitnuc_amd as bn
    k, nq = 23, 33
    rng = np.random.default_rng(78)
    n = sizes(k, 9)[4]
    pats1, _ = make_patterns(rng, k, nq, lead=0)
    pats2, _ = make_patterns(rng, k, nq, lead=3)
    taus = make_taus(k, nq, lead=2)
    codes1, codes2 = make_codes(rng, n, k, 9, pats1), make_codes(rng, n, k, 9, pats2)
    s1, s2 = ascii_of(rng, codes1), ascii_of(rng, codes2)
    want1, want2 = Want(codes1, k, pats1, taus), Want(codes2, k, pats2, taus)
    assert not np.array_equal(want1.counts, want2.counts)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = po.pack_codes(codes1)
        tw, wptr = _words_dev(w, 1)
        keep, dp = _patterns_dev(pats1, 1)
        dt = _u32_dev(taus)
        o1, o2 = _guarded64(nq), _guarded64(nq)
        c.kmer_pattern_count_multi_async(ptr, n, k, dp, dt, nq, o1)  # warm-up outside the capture: sizes the scratch
        c.kmer_pattern_count_multi_packed_async(wptr, w.size, n, k, dp, dt, nq, o2)
        c.sync()
        assert np.array_equal(_read64(o1, nq, "warm-up"), want1.counts) and np.array_equal(_read64(o2, nq, "warm-up"), want1.counts)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.kmer_pattern_count_multi_async(ptr, n, k, dp, dt, nq, o1)
                c.kmer_pattern_count_multi_packed_async(wptr, w.size, n, k, dp, dt, nq, o2)
            t[7:7 + n] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(po.pack_codes(codes2).view(np.int64)).to(tw.device)
            keep[1:] = torch.from_numpy(np.ascontiguousarray(np.stack(pats2)).reshape(-1).view(np.int32).copy()).to(keep.device)
            for _ in range(2):
                o1.fill_(FILL)
                o2.fill_(FILL)
                g.replay()
                c.sync()
                assert np.array_equal(_read64(o1, nq, "replay"), want2.counts) and np.array_equal(_read64(o2, nq, "replay"), want2.counts)
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_of_pattern_and_exact_calls_with_one_sync(ctx):
    """pattern and exact calls of all three families on one context, different query counts between neighbours (they share scratch slots 7, 8 and 9
    and rebuild their tables in-stream), one sync at the end, every result checked afterwards"""
    import torch
    k = 23
    rng = np.random.default_rng(606)
    jobs = []
    for i, nq in enumerate((5, 33, 1, 17, 16, 2)):
        n = 30_001 + 1000 * i
        off = (0, 7, 1)[i % 3]
        pats, singles = make_patterns(rng, k, nq, lead=i)
        if not singles:
            pats[0], singles = po.from_2bit(12345 + i, k), {0: 12345 + i}
        taus = make_taus(k, nq, lead=i)
        codes = make_codes(rng, n, k, (16 - off) % 16, pats)
        s = ascii_of(rng, codes)
        idx = sorted(singles)
        j = dict(i=i, nq=nq, n=n, pats=pats, taus=taus, idx=idx, want=Want(codes, k, pats, taus), a=_ascii_dev(s, off), w=po.pack_codes(codes),
                 dp=_patterns_dev(pats, i % 2), dt=_u32_dev(taus), dq=_u64_dev([singles[x] for x in idx]), dte=_u32_dev(taus[idx]), q0=singles[idx[0]],
                 counts=_guarded64(nq), ecounts=_guarded64(len(idx)), pos=_guarded64(nq), dist=_guarded8(nq), epos=_guarded64(len(idx)), edist=_guarded8(len(idx)),
                 hp=_guarded64(64), hd=_guarded8(64), nh=_guarded64(1), ehp=_guarded64(64), enh=_guarded64(1))
        j["wd"] = _words_dev(j["w"], i & 1)
        jobs.append(j)
    torch.cuda.synchronize()
    calls = 0
    for j in jobs:  # the queue: nothing waits between these calls
        ptr, n, nq, dp, dt, ne = j["a"][1], j["n"], j["nq"], j["dp"][1], j["dt"], len(j["idx"])
        wptr, nw = j["wd"][1], j["w"].size
        if j["i"] % 2 == 0:
            ctx.kmer_pattern_count_multi_async(ptr, n, k, dp, dt, nq, j["counts"])
            ctx.kmer_hdist_count_multi_packed_dev(wptr, nw, n, k, j["dq"], j["dte"], ne, j["ecounts"])
            ctx.kmer_pattern_best_packed_async(wptr, nw, n, k, dp, nq, j["pos"], j["dist"][1])
            ctx.kmer_hdist_best_async(ptr, n, k, j["dq"], ne, j["epos"], j["edist"][1])
            ctx.kmer_pattern_hits_async(ptr, n, k, j["pats"][j["idx"][0]], 3, j["hp"], j["hd"][1], 64, j["nh"])
            ctx.kmer_hdist_hits_packed_dev(wptr, nw, n, k, j["q0"], 3, j["ehp"], None, 64, j["enh"])
        else:
            ctx.kmer_hdist_hits_dev(ptr, n, k, j["q0"], 3, j["ehp"], None, 64, j["enh"])
            ctx.kmer_pattern_hits_packed_async(wptr, nw, n, k, j["pats"][j["idx"][0]], 3, j["hp"], j["hd"][1], 64, j["nh"])
            ctx.kmer_hdist_best_packed_async(wptr, nw, n, k, j["dq"], ne, j["epos"], j["edist"][1])
            ctx.kmer_pattern_best_async(ptr, n, k, dp, nq, j["pos"], j["dist"][1])
            ctx.kmer_hdist_count_multi_dev(ptr, n, k, j["dq"], j["dte"], ne, j["ecounts"])
            ctx.kmer_pattern_count_multi_packed_async(wptr, nw, n, k, dp, dt, nq, j["counts"])
        calls += 6
    assert calls == 36
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        want, nq, idx, tag = j["want"], j["nq"], j["idx"], j["i"]
        assert np.array_equal(_read64(j["counts"], nq, "counts"), want.counts), tag
        assert np.array_equal(_read64(j["ecounts"], len(idx), "exact counts"), want.counts[idx]), tag
        assert np.array_equal(_read64(j["pos"], nq, "pos"), want.pos) and np.array_equal(_read8(j["dist"][0], nq, "dist"), want.dist), tag
        assert np.array_equal(_read64(j["epos"], len(idx), "exact pos"), want.pos[idx]), tag
        assert np.array_equal(_read8(j["edist"][0], len(idx), "exact dist"), want.dist[idx]), tag
        hp, hd, total = po.hits(want.d[idx[0]], 3, 64)
        assert int(_read64(j["nh"], 1, "n_hits")[0]) == total == int(_read64(j["enh"], 1, "exact n_hits")[0]), tag
        assert np.array_equal(_read64(j["hp"], 64, "hits")[:hp.size], hp) and np.array_equal(_read8(j["hd"][0], 64, "hit_dist")[:hp.size], hd), tag
        assert np.array_equal(_read64(j["ehp"], 64, "exact hits")[:hp.size], hp), tag


def test_host_forms_above_the_cutoff_in_one_chunk():
    """2 * 10^6 bases and three patterns (6 * 10^6 window-pattern pairs, above the default cutoff of 2^20) on a context with the default dispatch: the
    six host forms and the PackedSequence methods run through the device in one chunk; IUPAC strings are accepted; an N in the reference is an error"""
    import bitnuc_amd as bn
    rng = np.random.default_rng(808)
    n, k = 2 * 10**6, 23
    guide = "".join("ACGT"[c] for c in rng.integers(0, 4, size=20))
    texts = [guide + "NGG", guide + "NRG", "N" * 20 + "NGG"]
    pats = [po.from_iupac(t) for t in texts]
    taus = np.array([3, 2, 0], dtype=np.uint32)
    codes = make_codes(rng, n, k, 0, pats)
    codes[n - k:] = [po.CODE[ch] for ch in guide] + [3, 2, 2]  # the last window is an exact site
    s = ascii_of(rng, codes)
    want = Want(codes, k, pats, taus)
    assert want.counts[0] >= 2 and want.counts[2] > 10_000
    words = po.pack_codes(codes, junk=0xDEADBEEFCAFEF00D) if n % 32 else po.pack_codes(codes)
    c = bn.Context(0)
    try:
        assert (n - k + 1) * 3 >= 1 << 20
        assert np.array_equal(c.kmer_pattern_count_multi(s, k, texts, taus), want.counts)
        assert np.array_equal(c.kmer_pattern_count_multi_packed(words, n, k, np.stack(pats), taus), want.counts)
        for got in (c.kmer_pattern_best(s, k, texts), c.kmer_pattern_best_packed(words, n, k, pats)):
            assert np.array_equal(got[0], want.pos) and np.array_equal(got[1], want.dist)
        hp, hd, total = po.hits(want.d[0], 3, 1 << 40)
        for got in (c.kmer_pattern_hits(s, k, texts[0], 3, with_dist=True), c.kmer_pattern_hits_packed(words, n, k, pats[0], 3, with_dist=True)):
            assert np.array_equal(got[0], hp) and np.array_equal(got[1], hd) and hp[-1] == n - k
        seq = bn.PackedSequence(s, c)
        assert np.array_equal(seq.kmer_pattern_count_multi(k, texts, taus), want.counts)
        assert np.array_equal(seq.kmer_pattern_best(k, texts)[0], want.pos)
        assert np.array_equal(seq.kmer_pattern_hits(k, texts[0], 3), hp)
        b = s.copy()
        b[n - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.kmer_pattern_count_multi(b, k, texts, taus)
        assert (ei.value.byte, ei.value.index) == (ord("N"), n - 5)
        del ei
        assert np.array_equal(c.kmer_pattern_count_multi(s, k, texts, taus), want.counts)  # the next call is clean
    finally:
        c.close()
