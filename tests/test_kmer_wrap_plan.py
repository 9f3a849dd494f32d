"""The case plan of the grid-wrap tests (tests/kmer_wrap_plan.py), checked without a GPU: its constants against the sources' text, the sizes it
picks against an independent walk of every wave's trips for five CU counts, and -- with the oracle alone, at the sizes of an 8-CU device -- the
condition that makes a trip-walk error visible: at the sensitive thresholds hardly any trip has the hit count of the trip one pass earlier."""
import os
import re

import numpy as np
import pytest

import kmer_wrap_plan as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnuc_amd", "csrc")
CUS = (8, 32, 64, 256, 304)
KS = (1, 16, 21, 31, 32)


def _const(fname, name):
    text = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"constexpr\s+(?:unsigned\s+)?(?:int|unsigned|size_t)\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, (fname, name)
    return int(m.group(1))


def test_plan_constants_are_the_sources():
    assert wp.K_BLOCK == _const("device_prims.h", "kBlock")
    assert wp.COUNT_ROUNDS == _const("runtime.h", "kCountRounds")
    assert wp.COUNT_GRID == _const("runtime.h", "kCountGrid")
    assert wp.MULTI_GRID == _const("kmer.hip", "kMultiGrid")
    assert wp.MULTI_BLOCK == _const("scan_multi_device.h", "kMultiBlock")
    assert wp.MULTI_ROUNDS == _const("scan_multi_device.h", "kMultiRounds")
    assert wp.MULTI_QB == _const("scan_multi_device.h", "kMultiQB")
    assert wp.HITS_TILE == _const("scan_hits_device.h", "kHitsTile")
    assert wp.HITS_ROUNDS == _const("scan_hits_device.h", "kHitsRounds")
    text = open(os.path.join(CSRC, "kmer.hip")).read()
    # the launchers the plan mirrors, as they are written
    assert "count3_t<kCountRounds>(c, ref, n, k, query, tau, res, slot, kCountGrid)" in text
    assert "bounded_grid(c, scan_rounds(n), (kBlock / 64) * U, per_cu)" in text
    assert "bounded_grid(c, scan_rounds(n, skip), (kBlock / 64) * 4, kCountGrid)" in text
    assert "bounded_grid(c, rounds, (kMultiBlock / 64) * kMultiRounds, kMultiGrid)" in text
    assert f"bounded_grid(c, scan_rounds(n), (kBlock / 64) * {wp.SCAN2_WAVE_ROUNDS}, {wp.SCAN2_GRID})" in text
    assert f"count_scan2_t<false, false, {wp.SCAN2_ROUNDS}, 0>" in text
    assert re.search(r"want = rounds / per_wg \+ 1, cap = \(unsigned long long\)c->num_cu \* \(unsigned\)per_cu", text)
    host = open(os.path.join(CSRC, "scan_mfma_host.h")).read()
    assert "return nr >= 1056 ? (nr - 32) >> 10 : 0;" in host
    for n in (0, 1055, 1056, 1057, 2079, 2080, 10**6):
        for skip in (0, 1, 15, 32):
            nr = max(n - skip, 0)
            assert wp.scan_rounds(n, skip) == (0 if nr < 1056 else (nr - 32) // 1024)


def _waves(kern, num_cu, rounds):
    """an independent walk: hand every trip to its wave, one by one -> (trips per wave, (wave, pass, length) of the last trip)"""
    grid = min(rounds // kern.per_wg + 1, num_cu * kern.per_cu)
    nwaves = grid * kern.waves
    ntrips = -(-rounds // kern.U)
    per = np.bincount(np.arange(ntrips) % nwaves, minlength=nwaves)
    t = ntrips - 1
    return per, (t % nwaves, t // nwaves, rounds - t * kern.U), grid


def _source_kernels():
    """the kernels' launch parameters from the sources' text, not from the plan's copies"""
    w, mw = _const("device_prims.h", "kBlock") // 64, _const("scan_multi_device.h", "kMultiBlock") // 64
    cr, cg = _const("runtime.h", "kCountRounds"), _const("runtime.h", "kCountGrid")
    mr, mg = _const("scan_multi_device.h", "kMultiRounds"), _const("kmer.hip", "kMultiGrid")
    K = wp.Kernel
    return {"count3": K("count3", w, cr, w * cr, cg, False), "packed_count3": K("packed_count3", w, 4, w * 4, cg, True),
            "multi": K("multi", mw, mr, mw * mr, mg, False), "packed_multi": K("packed_multi", mw, 4, mw * mr, mg, True),
            "scan2": K("scan2", w, 1, w * 4, 8, False)}  # (count_scan2_t's literals: test_plan_constants_are_the_sources)


def _check_plan(num_cu, k):
    if True:
        pl = wp.plan(num_cu, k)
        ks = _source_kernels()
        tile, hr = _const("scan_hits_device.h", "kHitsTile"), _const("scan_hits_device.h", "kHitsRounds")
        for name in ("count3", "packed_count3", "multi", "packed_multi"):
            kern, cs = ks[name], pl["cases"][name]
            R = num_cu * kern.per_cu * kern.waves * kern.U
            assert pl["P"][name] == R * 1024
            if num_cu == 256:
                assert pl["P"][name] == (50_331_648 if "count3" in name else 12_582_912)
            by_rounds = {}
            for c in cs:
                by_rounds.setdefault(c.rounds, []).append(c)
            want = [R + d for d in range(-1, 6)] + [2 * R + d for d in range(-1, 6)]
            assert set(want) < set(by_rounds) and any(3 * R + R // 2 <= r <= 3 * R + R // 2 + 4 for r in by_rounds)
            seen_partial = set()
            most = set()
            for r, group in by_rounds.items():
                per, (lw, lpass, llen), grid = _waves(kern, num_cu, r)
                assert grid == num_cu * kern.per_cu  # the grid is full: a pass is R rounds
                most.add(int(per.max()))
                if lpass >= 1 and llen < kern.U:
                    seen_partial.add((lpass, llen))
                for base, passes in ((R, 1), (2 * R, 2)):
                    if base < r <= base + kern.U:  # the first wave's trip number passes + 1, alone, of r - base rounds
                        assert per[0] == passes + 1 and per[1:].max() == passes and (lw, lpass, llen) == (0, passes, r - base)
                    if r == base + kern.U + 1:
                        assert per[0] == per[1] == passes + 1 and (lw, lpass, llen) == (1, passes, 1)
                    if r in (base - 1, base):
                        assert per.max() == passes and lpass == passes - 1 and llen == (kern.U - 1 if r == base - 1 else kern.U)
                # per round count and alignment: the smallest and the largest n with that count, one in between, and the k - 1 edge
                aligns = {}
                for c in group:
                    aligns.setdefault((c.o % 16) if not kern.packed else (c.o // 32) % 2, []).append(c)
                assert set(aligns) == ({0} if name == "count3" else set(wp.ASCII_OFFSETS) if name == "multi" else {0, 1})
                for al, g in aligns.items():
                    ns = sorted(c.n - c.skip for c in g)
                    assert len(ns) == 4 and ns[0] == 1024 * r + 32 and ns[-1] == 1024 * r + 1055
                    assert wp.scan_rounds(ns[0] - 1) == r - 1 and wp.scan_rounds(ns[-1] + 1) == r + 1
                    assert (1024 * r + 2 * k - 2 in ns) if 2 * k - 2 > 32 else (1024 * r + 32 + max(k - 1, 1) in ns)
                    for c in g:
                        assert c.skip == ((32 * al) if kern.packed else (16 - al) % 16 if name == "multi" else 0)
                        assert c.o % 32 == 0 or not kern.packed
            assert {2, 3, 4} <= most
            if kern.U > 1:  # a partial last trip of every length on the second and on the third pass
                assert {(p, m) for p in (1, 2) for m in range(1, kern.U)} <= seen_partial
            limit = pl["length"] if "count3" in name else pl["length_small"]
            assert all(c.o + c.n <= limit and c.n >= k for c in cs)
        # the bit-plane count rides along at the matrix-core count's sizes with o mod 16 in {1, 7, 15}: full grid, several one-round trips per wave
        s2 = pl["cases"]["scan2"]
        assert {c.o % 16 for c in s2} == {1, 7, 15} and len(s2) == 3 * len(pl["cases"]["count3"])
        for c in s2[:: max(1, len(s2) // 12)]:
            per, _, grid = _waves(ks["scan2"], num_cu, c.rounds)
            assert grid == num_cu * 8 and per.min() >= 3
        assert all(c.o + c.n <= pl["length"] for c in s2)
        # hit lists: per-trip counts (trips + head + tail) just below, at and just above one, two and three tiles, at every alignment
        for name, aligns in (("hits", set(wp.ASCII_OFFSETS)), ("packed_hits", {0, 1})):
            got = {}
            for c in pl["cases"][name]:
                ntr = -(-wp.scan_rounds(c.n, c.skip) // hr) + 2
                al = c.o % 16 if name == "hits" else (c.o // 32) % 2
                assert c.skip == ((16 - al) % 16 if name == "hits" else 32 * al) and c.o + c.n <= pl["length_small"]
                got.setdefault(ntr, set()).add(al)
            assert set(got) == {t * tile + d for t in (1, 2, 3) for d in (-1, 0, 1)}
            assert all(a == aligns for a in got.values())
        assert any(wp.scan_rounds(c.n, c.skip) % hr for c in pl["cases"]["hits"])
        # planted copies: inside the sequence, apart, and where the plan says they are
        pos = sorted(pl["plants"])
        assert pos[-1] + k <= pl["length"] and all(b - a >= k for a, b in zip(pos, pos[1:]))
        P1, P2 = pl["P"]["count3"], pl["P"]["multi"]
        assert {wp.ANCHOR, wp.ANCHOR + P1 - 1, wp.ANCHOR + 2 * P1, wp.ANCHOR + 2 * P2 - 1, wp.ANCHOR + 3 * P2} <= set(pos)
        assert wp.ANCHOR + (tile - 1) * hr * 1024 - 1 in pos and wp.ANCHOR + (2 * tile - 1) * hr * 1024 in pos
        assert 3.5 <= pl["length"] / P1 <= 3.7 or pl["length"] == pl["length_small"] + 64  # (a small device: the hit lists' three tiles are longer)
        for fam, (r, nb) in pl["dedicated"].items():
            assert wp.scan_rounds(nb) == r and wp.ANCHOR + nb <= (pl["length"] if fam == "count3" else pl["length_small"])


@pytest.mark.parametrize("num_cu", CUS)
def test_plan_reaches_second_and_third_trips(num_cu):
    for k in KS:
        _check_plan(num_cu, k)


@pytest.mark.parametrize("name,value", [("COUNT_GRID", 24), ("COUNT_GRID", 6), ("COUNT_ROUNDS", 2), ("MULTI_BLOCK", 512), ("MULTI_GRID", 2),
                                        ("K_BLOCK", 512), ("HITS_TILE", 2048), ("HITS_ROUNDS", 2)])
def test_plan_check_fails_when_a_constant_moves(monkeypatch, name, value):
    """the checks above walk the kernels as the SOURCES launch them: a plan built from another constant no longer passes them"""
    _check_plan(256, 31)
    monkeypatch.setattr(wp, name, value)
    with pytest.raises(AssertionError):
        _check_plan(256, 31)


@pytest.mark.parametrize("k", KS)
def test_generated_data_makes_a_trip_walk_error_visible(oracle, k):
    """The sensitivity condition on the oracle's distances alone, at the sizes of an 8-CU device: for each sensitive threshold and each kernel
    at most 5 % of the trips have the hit count of the same wave's trip one pass earlier, at most 5 % have no hit or only hits; for every
    query of the multi-query counts; and every planted copy is an exact match."""
    num_cu = 8
    pl = wp.plan(num_cu, k)
    q, _ = wp.make_query(k, 0xC0FFEE + k)
    qs = wp.multi_queries(q)
    L = min(pl["length"], 4 * pl["P"]["count3"])
    s = wp.make_sequence(L, q, 0x5EED + k, pl["plants"])
    assert set(np.unique(s)) <= set(b"ACGTacgt") and 0.25 < float(np.mean(s & 0x20 != 0)) < 0.35
    dist = oracle.kmer_hdist_scan_threaded(s, k, qs[0][1])
    assert np.array_equal(dist[:100_000], oracle.kmer_hdist_scan(s[:100_000 + k - 1], k, qs[0][1]))
    figures = wp.check_sensitivity(dist, k, num_cu)
    print(k, {key: (round(a, 4), round(b, 4)) for key, (a, b) in figures.items()})
    for p in pl["plants"]:
        if p + k <= L:
            assert dist[p] == 0, (p, pl["plants"][p])
    Ls = min(L, 6 * pl["P"]["multi"])
    for codes, word in qs[1:]:
        d = oracle.kmer_hdist_scan_threaded(s[:Ls], k, word)
        wp.check_sensitivity(d, k, num_cu, names=("multi",))
    # the boundary thresholds are not what the condition is about: tau >= k counts every window
    assert int((dist <= k).sum()) == dist.size
    # the packed form of the data is the oracle's encoding
    assert np.array_equal(wp.pack_words(s[:100_003]), oracle.encode(s[:100_003]))
