"""GPU tests of the sliding k-mer counts and hit lists at the sizes where their second-level structure starts to work (-m gpu): the bounded grids
of kmer_count3_mfma_kernel / packed_count3_mfma_kernel (12 workgroups per CU) and of the multi-query kernels (one 12-wave workgroup per CU) wrap,
so a wave walks a second, third and fourth trip, loading each into the registers the previous one has just left, with a partial last trip of every
length on a later pass; the unaligned count's one-round trips ride along at the same sizes; and the hit lists' per-trip counts fill more than one
tile of their two-level scan.

One seeded sequence per k (tests/kmer_wrap_plan.py: the query repeated end to end under a drifting mutation rate, mixed case, exact copies
planted at the pass and tile boundaries), ONE oracle scan of it per query on the host cores, and every case is a sub-range s[o : o + n]: its
expected distances are dist[o : o + n - k + 1], its pointer alignment o mod 16 (ASCII) or (o / 32) mod 2 words (packed).  Every expected value
is derived from the oracle's distances (torch only sums / selects them on the device); none comes from another call of the library.  Before
the first launch the oracle's distances alone must show that a trip counted in place of another would be seen (kmer_wrap_plan.check_sensitivity).

The sizes follow the device: plan(ctx.get("num_cu")).  On 256 CUs: 3.6 passes of 50 331 648 windows for the single counts, of 12 582 912 for
the multi-query counts, and 3 tiles of 16 777 216 windows for the hit lists."""
import numpy as np
import pytest

import bitnuc_amd as bn
import kmer_wrap_plan as wp

pytestmark = pytest.mark.gpu

KS = (1, 16, 21, 31, 32)
NQS = (1, 16, 17, 40)  # grid.y = 1, 1, 2, 3; 17 and 40 end in a partial query block
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
DIST_FILL = 0xEE
_worlds = {}


class World:
    pass


@pytest.fixture(scope="module", autouse=True)
def _drop_worlds():
    yield
    _worlds.clear()


def _world(ctx, oracle, k):
    """the sequence of this k, the oracle's distances per query (host and device), the packed words, the plan"""
    if k in _worlds:
        return _worlds[k]
    import torch
    w = World()
    w.k, w.num_cu = k, int(ctx.get("num_cu"))
    assert w.num_cu > 0
    w.pl = pl = wp.plan(w.num_cu, k)
    q, _ = wp.make_query(k, 0xC0FFEE + k)
    w.qs = wp.multi_queries(q)
    w.query = w.qs[0][1]
    s = wp.make_sequence(pl["length"], q, 0x5EED + k, pl["plants"])
    dists = [oracle.kmer_hdist_scan_threaded(s, k, w.query)]
    dists += [oracle.kmer_hdist_scan_threaded(s[:pl["length_small"]], k, word) for _, word in w.qs[1:]]
    # the condition, on the oracle alone, before the GPU sees the data: a miss is a failure of the test
    w.figures = wp.check_sensitivity(dists[0], k, w.num_cu)
    for d in dists[1:]:
        wp.check_sensitivity(d, k, w.num_cu, names=("multi",))
    ntr = (dists[0].size - wp.ANCHOR) // 4096
    for tau in wp.sensitive_taus(k):  # the hit lists: a trip against the trip one tile of per-trip counts earlier
        same, flat = wp.sensitivity(dists[0], tau, wp.ANCHOR, 4096, min(ntr, 3 * wp.HITS_TILE), wp.HITS_TILE)
        assert same <= wp.SENSITIVITY_CAP and flat <= wp.SENSITIVITY_CAP, ("hits", k, tau, same, flat)
    for p, what in pl["plants"].items():
        assert dists[0][p] == 0, (p, what)
    w.s_dev = torch.from_numpy(s).to("cuda:0")
    w.words_dev = torch.from_numpy(wp.pack_words(s).view(np.int64)).to("cuda:0")
    w.d_dev = [torch.from_numpy(d).to("cuda:0") for d in dists]
    assert w.s_dev.data_ptr() % 16 == 0 and w.words_dev.data_ptr() % 16 == 0
    w.taus = sorted(set(wp.boundary_taus(k)) | set(wp.sensitive_taus(k)))
    torch.cuda.synchronize()
    _worlds[k] = w
    return w


def _le(d, tau):
    return d <= min(int(tau), 255)


def _want_counts(w, j, o, nwin, taus):
    """windows of s[o : o + nwin + k - 1] within tau of query j, per tau: from the oracle's distances"""
    import torch
    d = w.d_dev[j][o:o + nwin]
    assert d.numel() == nwin
    return [int(x) for x in torch.stack([_le(d, t).sum() for t in taus]).cpu()]


def sync_error(ctx):
    try:
        ctx.sync()
        return None
    except bn.NucleotideError as e:
        return (e.kind, getattr(e, "byte", None), getattr(e, "index", None))


def _count_single(ctx, w, packed, o, n, taus):
    """-> the counts per tau; the result cells sit between guard cells that must stay"""
    import torch
    res = torch.full((2 * len(taus) + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for i, tau in enumerate(taus):
        if packed:
            ctx.kmer_hdist_count_packed_dev(w.words_dev.data_ptr() + 8 * (o // 32), (n + 31) // 32, n, w.k, w.query, tau, res[2 * i + 1:])
        else:
            ctx.kmer_hdist_count_dev(w.s_dev.data_ptr() + o, n, w.k, w.query, tau, res[2 * i + 1:])
    ctx.sync()
    got = res.cpu().numpy()
    assert (got[0::2] == -1).all(), "a guard cell beside the count was written"
    return [int(x) for x in got[1::2]]


@pytest.mark.parametrize("k", KS)
def test_single_counts_across_passes(ctx, oracle, k):
    """kmer_hdist_count_dev at o mod 16 = 0 (the matrix-core count) and 1 / 7 / 15 (the bit-plane count), kmer_hdist_count_packed_dev at both word
    alignments: rounds R - 1 .. R + 5 and 2 R - 1 .. 2 R + 5 of the pass R, and 3.5 R + 1; per round count the smallest and the largest n, the
    k - 1 edge and one in between; tau in {0, 1, the sensitive thresholds, k - 1, k, 2^32 - 1}."""
    w = _world(ctx, oracle, k)
    fails, ran = [], 0
    for name in ("count3", "scan2", "packed_count3"):
        for c in w.pl["cases"][name]:
            nwin = c.n - k + 1
            got = _count_single(ctx, w, name == "packed_count3", c.o, c.n, w.taus)
            want = _want_counts(w, 0, c.o, nwin, w.taus)
            ran += 1
            for tau, g, e in zip(w.taus, got, want):
                if g != e:
                    fails.append(f"{name} o={c.o} n={c.n} rounds={c.rounds} k={k} tau={tau}: count {g}, oracle {e} ({g - e:+d})")
    print(f"k={k}: {ran} sub-ranges x {len(w.taus)} thresholds on {w.num_cu} CUs, sequence of {w.pl['length']} bases; sensitivity {w.figures}")
    assert ran == len(w.pl["cases"]["count3"]) * 4 + len(w.pl["cases"]["packed_count3"])
    assert not fails, "\n".join(fails[:30]) + f"\n({len(fails)} failing (case, tau) of {ran} cases)"


def _multi_slots(w, nq):
    """slot i: query i mod (distinct queries), the thresholds taken in turn so that a query returns with another threshold"""
    nd = len(w.qs)
    return [(i % nd, w.taus[(i // nd + i) % len(w.taus)]) for i in range(nq)]


@pytest.mark.parametrize("k", KS)
def test_multi_counts_across_passes(ctx, oracle, k):
    """kmer_hdist_count_multi_dev at o mod 16 in {0, 1, 7, 15} (skip = 16 - o mod 16) and kmer_hdist_count_multi_packed_dev at both word alignments,
    around one, two and three and a half passes of the one-workgroup-per-CU grid, with 1, 16, 17 and 40 queries (grid.y = 1, 1, 2, 3; 16 per-lane
    counters live across the trips): every count against the oracle's scan for that query, guard cells after counts[nq]."""
    import torch
    w = _world(ctx, oracle, k)
    dev = {}
    for nq in NQS:
        slots = _multi_slots(w, nq)
        dq = torch.from_numpy(np.array([w.qs[j][1] for j, _ in slots], dtype=np.uint64).view(np.int64)).to("cuda:0")
        dt = torch.from_numpy(np.array([t for _, t in slots], dtype=np.uint32).view(np.int32)).to("cuda:0")
        dev[nq] = (slots, dq, dt)
    fails, ran = [], 0
    for name in ("multi", "packed_multi"):
        for idx, c in enumerate(w.pl["cases"][name]):
            vi, al, ri = (idx % 4, (idx // 4) % 4, idx // 16) if name == "multi" else (idx % 4, (idx // 4) % 2, idx // 8)
            nq = NQS[(vi + al + ri) % 4]
            slots, dq, dt = dev[nq]
            nwin = c.n - k + 1
            counts = torch.full((nq + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            if name == "multi":
                ctx.kmer_hdist_count_multi_dev(w.s_dev.data_ptr() + c.o, c.n, k, dq, dt, nq, counts)
            else:
                ctx.kmer_hdist_count_multi_packed_dev(w.words_dev.data_ptr() + 8 * (c.o // 32), (c.n + 31) // 32, c.n, k, dq, dt, nq, counts)
            ctx.sync()
            got = counts.cpu().numpy()
            ran += 1
            if not (got[nq:] == FILL).all():
                fails.append(f"{name} o={c.o} n={c.n} nq={nq}: counts written after n_queries")
            table = {}
            for j in sorted({j for j, _ in slots}):
                ts = sorted({t for jj, t in slots if jj == j})
                table.update({(j, t): e for t, e in zip(ts, _want_counts(w, j, c.o, nwin, ts))})
            for i, (j, t) in enumerate(slots):
                if int(got[i]) != table[(j, t)]:
                    fails.append(f"{name} o={c.o} n={c.n} rounds={c.rounds} k={k} nq={nq} slot {i} (query {j}, tau {t}): count {int(got[i])}, "
                                 f"oracle {table[(j, t)]} ({int(got[i]) - table[(j, t)]:+d})")
    print(f"k={k}: {ran} multi-query calls, {len(w.qs)} distinct queries")
    assert ran == len(w.pl["cases"]["multi"]) + len(w.pl["cases"]["packed_multi"])
    assert not fails, "\n".join(fails[:30]) + f"\n({len(fails)} failures in {ran} cases)"


def _hits_call(ctx, w, packed, o, n, tau, cap, with_dist):
    import torch
    pos = torch.full((cap + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    hd = torch.full((cap + GUARD,), DIST_FILL, dtype=torch.uint8, device="cuda:0") if with_dist else None
    nh = torch.full((3,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    if packed:
        ctx.kmer_hdist_hits_packed_dev(w.words_dev.data_ptr() + 8 * (o // 32), (n + 31) // 32, n, w.k, w.query, tau, pos, hd, cap, nh[1:])
    else:
        ctx.kmer_hdist_hits_dev(w.s_dev.data_ptr() + o, n, w.k, w.query, tau, pos, hd, cap, nh[1:])
    return pos, hd, nh


def _hits_check(pos, hd, nh, cap, want, want_d, tag):
    """-> a failure text or None; everything compared on the device"""
    total = int(want.numel())
    h = [int(x) for x in nh.cpu()]
    if h != [-1, total, -1]:
        return f"{tag}: n_hits cell {h}, oracle {total}"
    g = min(cap, total)
    if not bool((pos[g:] == FILL).all()):
        return f"{tag}: positions written at or beyond min(cap, total) = {g}"
    if not bool((pos[:g] == want[:g]).all()):
        i = int((pos[:g] != want[:g]).nonzero()[0])
        return f"{tag}: hit {i} is window {int(pos[i])}, oracle {int(want[i])}"
    if hd is not None:
        if not bool((hd[g:] == DIST_FILL).all()):
            return f"{tag}: distances written at or beyond min(cap, total) = {g}"
        if not bool((hd[:g] == want_d[:g]).all()):
            i = int((hd[:g] != want_d[:g]).nonzero()[0])
            return f"{tag}: distance of hit {i} (window {int(want[i])}) is {int(hd[i])}, oracle {int(want_d[i])}"
    return None


@pytest.mark.parametrize("k", KS)
def test_hit_lists_across_tiles(ctx, oracle, k):
    """kmer_hdist_hits_dev at o mod 16 in {0, 1, 7, 15} and kmer_hdist_hits_packed_dev at both word alignments with trips + 2 per-trip counts just
    below, at and just above one, two and three tiles of 4096: positions and distances against the windows of the oracle's scan within tau, at a
    sensitive tau (an irregular, moderately dense to dense pattern across the tile boundaries) and at tau = 0 (the planted copies among them);
    cap in {total + 5, total, inside the second tile's hits, the hits before the third tile, 1, 0}, with and without hit_dist; guard elements
    after min(cap, total); *n_hits = total whatever cap."""
    import torch
    w = _world(ctx, oracle, k)
    sens = wp.sensitive_taus(k)
    fails, ran = [], 0
    for name in ("hits", "packed_hits"):
        for idx, c in enumerate(w.pl["cases"][name]):
            nwin = c.n - k + 1
            d = w.d_dev[0][c.o:c.o + nwin]
            for tau in sorted({sens[idx % len(sens)], 0}):
                want = torch.nonzero(_le(d, tau)).flatten()
                want_d = d[want]
                total = int(want.numel())
                b1, b2 = c.skip + wp.tile_first_window(1), c.skip + wp.tile_first_window(2)
                before = lambda x: int((want < x).sum())  # noqa: E731
                inside2 = before((b1 + b2) // 2) if nwin > b2 else before(b1 + (nwin - b1) // 2) if nwin > b1 else total // 2
                caps = [total + 5, total, inside2, before(b2), 1, 0]
                for ci, cap in enumerate(caps):
                    for with_dist in (True, False):
                        tag = f"{name} o={c.o} n={c.n} rounds={c.rounds} ({c.tag}) k={k} tau={tau} cap={cap} hit_dist={with_dist}"
                        pos, hd, nh = _hits_call(ctx, w, name == "packed_hits", c.o, c.n, tau, cap, with_dist)
                        ctx.sync()
                        f = _hits_check(pos, hd, nh, cap, want, want_d, tag)
                        ran += 1
                        if f:
                            fails.append(f)
                        del pos, hd
    # the planted copies are hits at tau = 0 of a sub-range that starts at ANCHOR: both sides of a tile boundary
    r, nb = w.pl["dedicated"]["hits"]
    for o in (wp.ANCHOR, wp.ANCHOR - 1, wp.ANCHOR - 7, wp.ANCHOR - 15):
        n = wp.ANCHOR + nb - o
        d = w.d_dev[0][o:o + n - k + 1]
        want = torch.nonzero(d == 0).flatten()
        rel = sorted(p - o for p in w.pl["plants"] if o <= p and p - o + k <= n)
        assert len(rel) >= 5 and rel[-1] == n - k and (rel[0] == 0) == (o == wp.ANCHOR)  # the first and the last window of the range among them
        assert bool(torch.isin(torch.tensor(rel, device="cuda:0"), want).all())
        pos, hd, nh = _hits_call(ctx, w, False, o, n, 0, int(want.numel()), True)
        ctx.sync()
        f = _hits_check(pos, hd, nh, int(want.numel()), want, d[want], f"hits (planted copies) o={o} n={n} k={k} tau=0")
        ran += 1
        if f:
            fails.append(f)
    print(f"k={k}: {ran} hit-list calls")
    assert ran == 12 * 2 * (len(w.pl["cases"]["hits"]) + len(w.pl["cases"]["packed_hits"])) + 4 or k == 1
    assert not fails, "\n".join(fails[:30]) + f"\n({len(fails)} failures in {ran} calls)"


@pytest.mark.parametrize("k", KS)
def test_counts_see_the_planted_copies(ctx, oracle, k):
    """Sub-ranges whose rounds start at ANCHOR (o = 16, 15, 9, 1), three and a half passes long: the exact copies planted at the last window of a
    pass, the first window of a pass and across the halo between two passes are among the windows at distance 0, and the counts at tau = 0 and
    at the sensitive thresholds are the oracle's -- the single count, the packed count (o = 0 and 32) and 40 queries at once."""
    import torch
    w = _world(ctx, oracle, k)
    taus = sorted({0, *wp.sensitive_taus(k)})
    for fam in ("count3", "multi"):
        r, nb = w.pl["dedicated"][fam]
        for o in (wp.ANCHOR, wp.ANCHOR - 1, wp.ANCHOR - 7, wp.ANCHOR - 15):
            n = wp.ANCHOR + nb - o
            rel = sorted(p - o for p in w.pl["plants"] if o <= p and p - o + k <= n)
            assert len(rel) >= 7 and rel[-1] == n - k and (rel[0] == 0) == (o == wp.ANCHOR) and bool((w.d_dev[0][o:o + n - k + 1][torch.tensor(rel, device="cuda:0")] == 0).all())
            if fam == "count3":
                assert _count_single(ctx, w, False, o, n, taus) == _want_counts(w, 0, o, n - k + 1, taus), (fam, o, n)
            else:
                slots = _multi_slots(w, 40)
                dq = torch.from_numpy(np.array([w.qs[j][1] for j, _ in slots], dtype=np.uint64).view(np.int64)).to("cuda:0")
                dt = torch.from_numpy(np.array([t for _, t in slots], dtype=np.uint32).view(np.int32)).to("cuda:0")
                counts = torch.full((40 + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                ctx.kmer_hdist_count_multi_dev(w.s_dev.data_ptr() + o, n, k, dq, dt, 40, counts)
                ctx.sync()
                got = counts.cpu().numpy()
                assert (got[40:] == FILL).all()
                for i, (j, t) in enumerate(slots):
                    assert int(got[i]) == _want_counts(w, j, o, n - k + 1, [t])[0], (fam, o, n, i, j, t)
        for o in (0, 32):
            n = wp.ANCHOR + nb - o
            assert _count_single(ctx, w, True, o, n, taus) == _want_counts(w, 0, o, n - k + 1, taus), (fam, "packed", o, n)


@pytest.mark.parametrize("k", KS)
def test_invalid_bytes_on_later_passes(ctx, oracle, k):
    """Plant, run, restore: an N in pass 2 and a later x in pass 3; one in pass 3 only; one in pass 2 under an unaligned pointer; one in the partial
    last trip.  kmer_hdist_count_dev, kmer_hdist_count_multi_dev with 40 queries (three query blocks: reported once, the first in sequence
    order) and kmer_hdist_hits_dev report (byte, index relative to the pointer passed) of the first plant; the next sync reports nothing; the
    next valid call on the same context is correct (ticket and accumulator left clean)."""
    import torch
    w = _world(ctx, oracle, k)
    tau = wp.sensitive_taus(k)[-1]
    slots = _multi_slots(w, 40)
    dq = torch.from_numpy(np.array([w.qs[j][1] for j, _ in slots], dtype=np.uint64).view(np.int64)).to("cuda:0")
    dt = torch.from_numpy(np.array([t for _, t in slots], dtype=np.uint32).view(np.int32)).to("cuda:0")

    def run(fam, ptr, n):
        if fam == "count3":
            res = torch.full((3,), -1, dtype=torch.int64, device="cuda:0")
            ctx.kmer_hdist_count_dev(ptr, n, k, w.query, tau, res[1:])
            return lambda o: [int(x) for x in res.cpu()] == [-1, _want_counts(w, 0, o, n - k + 1, [tau])[0], -1]
        if fam == "multi":
            counts = torch.full((40 + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
            ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, 40, counts)
            return lambda o: [int(x) for x in counts.cpu()[:40]] == [_want_counts(w, j, o, n - k + 1, [t])[0] for j, t in slots]
        nh = torch.full((3,), -1, dtype=torch.int64, device="cuda:0")
        ctx.kmer_hdist_hits_dev(ptr, n, k, w.query, tau, None, None, 0, nh[1:])
        return lambda o: [int(x) for x in nh.cpu()] == [-1, _want_counts(w, 0, o, n - k + 1, [tau])[0], -1]

    fails = []
    for fam in ("count3", "multi", "hits"):
        rounds, nb = w.pl["dedicated"][fam]
        Pw = w.pl["P"][fam] if fam != "hits" else wp.tile_first_window(1) + 4096  # the hit lists: "pass" = a tile of per-trip counts
        last = 1024 * (rounds - 1)  # the partial last trip's only round (rounds = 3.5 R + 1; the hit lists: the last trip has three)
        plantings = [
            ("N in pass 2, x in pass 3", wp.ANCHOR, [(Pw + 12345, ord("N")), (2 * Pw + 777, ord("x"))]),
            ("pass 3 only", wp.ANCHOR, [(2 * Pw + 5 * 4096 + 1000, 0x00)]),
            ("pass 2, pointer + 9", wp.ANCHOR - 7, [(Pw + 4321, ord("n"))]),
            ("pass 2, pointer + 1, two plants in one trip", wp.ANCHOR - 15, [(Pw + 4096 * 3 + 2050, 0xFF), (Pw + 4096 * 3 + 3000, ord("N"))]),
            ("the partial last trip", wp.ANCHOR, [(last + 500, ord("U"))]),
        ]
        for what, o, plants in plantings:
            n = wp.ANCHOR + nb - o
            assert all(wp.ANCHOR + rel < o + n - 64 for rel, _ in plants)
            keep = [int(w.s_dev[wp.ANCHOR + rel]) for rel, _ in plants]
            for rel, byte in plants:
                w.s_dev[wp.ANCHOR + rel] = byte
            torch.cuda.synchronize()
            try:
                run(fam, w.s_dev.data_ptr() + o, n)
                got = sync_error(ctx)
                again = sync_error(ctx)
            finally:
                for (rel, _), b in zip(plants, keep):
                    w.s_dev[wp.ANCHOR + rel] = b
                torch.cuda.synchronize()
            want = ("InvalidBase", plants[0][1], wp.ANCHOR + plants[0][0] - o)
            tag = f"{fam} k={k} o={o} n={n} ({what})"
            if got != want:
                fails.append(f"{tag}: error {got}, planted {want}")
            if again is not None:
                fails.append(f"{tag}: the next sync reports {again}")
            ok = run(fam, w.s_dev.data_ptr() + o, n)
            err = sync_error(ctx)
            if err is not None or not ok(o):
                fails.append(f"{tag}: the next valid call: error {err}, result equal to the oracle's: {err is None and ok(o)}")
    assert not fails, "\n".join(fails)
