"""CPU checks of tests/alphabet.py: the byte classes and the coverage reject_plan promises to tests/test_gpu_alphabet.py."""
from collections import defaultdict

import numpy as np
import pytest

import alphabet as ab


def test_class_sizes_and_members():
    assert len(ab.VALID) == 8 and bytes(ab.VALID) == b"ACGTacgt"
    assert len(ab.INVALID_VALID_SELECTOR) == 120 and len(ab.INVALID_OTHER) == 128 and len(ab.INVALID) == 248
    assert set(ab.VALID) | set(ab.INVALID_VALID_SELECTOR) | set(ab.INVALID_OTHER) == set(range(256))
    assert not set(ab.INVALID_VALID_SELECTOR) & set(ab.INVALID_OTHER)
    for b in b"YSWKDyswkd":  # IUPAC ambiguity codes that share their low three bits with a base
        assert b in ab.INVALID_VALID_SELECTOR, chr(b)
    for b in b"NnRrMm\n >@0":
        assert b in ab.INVALID_OTHER, chr(b)
    assert {b & 7 for b in ab.INVALID_VALID_SELECTOR} == {b & 7 for b in ab.VALID} == {1, 3, 4, 7}
    assert {b & 7 for b in ab.INVALID_OTHER} == {0, 2, 5, 6}
    # the residues that class leaves once the case bit and the selector are taken away: fifteen of the sixteen values of bits 3, 4, 6, 7 per selector
    # group, each of the four mask bits 0x08, 0x10, 0x40, 0x80 the only difference from a base for some byte
    for bit in (0x08, 0x10, 0x40, 0x80):
        assert any((b ^ bit) in ab.VALID for b in ab.INVALID_VALID_SELECTOR), hex(bit)
    for b in ab.INVALID:
        assert ab.CLASS_OF[ab.other_class(b, b)] not in ("valid", ab.CLASS_OF[b])


def test_kernel_constants_match_the_sources():
    """the tiling constants the GPU file's regions are derived from, read back from the sources' text"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bitnuc_amd", "csrc")
    for name, (value, src) in ab.KERNEL_CONSTANTS.items():
        text = open(os.path.join(csrc, src)).read()
        m = re.search(r"constexpr\s+(?:unsigned|int)\s+" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == value, (name, src)
    assert all(ab.KERNEL_CONSTANTS[k][0] == ab.TRIP for k in ("kSlide2Rounds", "kScanSegRounds", "kCountRounds", "kHitsRounds", "kMultiRounds"))
    text = open(os.path.join(csrc, "codec.hip")).read()
    enc = re.search(r"kDefaultEnc == (\d+)", text).group(1)
    u, b = re.search(r"X\(" + enc + r",\s*(\d+),\s*(\d+),", text).groups()
    assert int(u) * int(b) * ab.GROUP == ab.ENCODE_TILE
    host = open(os.path.join(csrc, "scan_mfma_host.h")).read()
    assert "nr >= 1056 ? (nr - 32) >> 10 : 0" in host  # scan_rounds
    assert [ab.scan_rounds(n, s) for n, s in ((1055, 0), (1056, 0), (1056, 7), (6509, 0), (6509 + 9, 9))] == [0, 1, 0, 6, 6]
    assert [ab.rounds992(n) for n in (1023, 1024, 2015, 2016, 2300)] == [0, 1, 1, 2, 2]
    # the search kernels (tests/alphabet_search.py): the chunks, trips, waves and query groups its shapes rest on, and the header's span limit
    import alphabet_search as als
    kc = als.KC
    assert kc["kEdistRefChunk"] % kc["kEdistRefTrip"] == 0 and kc["kEdistRefLead"] % kc["kEdistRefTrip"] == 0 and als.EDIST_REF_N % kc["kEdistRefTrip"]
    assert kc["kAnchorBlock"] // 64 * als.WAVE == 256 and als.A_COUNT % als.WAVE and als.E_COUNT % kc["kEdistBlock"] and als.E_COUNT > kc["kEdistBlock"]
    assert als.Q5 % kc["kEdistInterleave"] == 1 and als.Q17 == ab.KERNEL_CONSTANTS["kMultiQB"][0] + 1
    assert 20 < kc["kReadsMinPeriod"] <= 150
    header = open(os.path.join(os.path.dirname(csrc), "..", "include", "bitnuc_hip.h")).read()
    assert int(re.search(r"#define\s+BITNUC_ANCHOR_MAX_SPAN\s+(\d+)", header).group(1)) == als.ANCHOR_MAX_SPAN
    assert f"the piece of `len` <= {als.PIECE} span bytes" in open(os.path.join(csrc, "scan_anchored_device.h")).read()
    dwords = re.search(r"struct EdistPieceAscii \{ uint32_t d\[(\d+)\]; \}", open(os.path.join(csrc, "scan_edist_best_device.h")).read()).group(1)
    assert int(dwords) == als.EDIST_PIECE // 4 + 1  # the aligned dwords that hold a piece of 64 bytes at any alignment


REGION_SETS = [
    [("body", range(0, 4096))],
    [("body", range(0, 6144)), ("halo", range(6144, 6176)), ("tail", range(6176, 6500))],
    [("head", range(0, 7)), ("body", range(7, 4103)), ("halo", range(4103, 4135)), ("tail", range(4135, 4400))],
    [("first", [p for p in range(0, 41 * 256) if p % 41 < 21]), ("rest", [p for p in range(41 * 256, 41 * 600) if p % 41 < 21])],
    [("head", range(5, 16)), ("tail", range(4176, 4187))],
]


@pytest.mark.parametrize("regions", REGION_SETS, ids=lambda r: "+".join(n for n, _ in r))
def test_reject_plan_coverage(regions):
    plan = list(ab.reject_plan(regions))
    assert len(plan) == 992
    pairs = [(b, p % 4) for b, p, _ in plan]
    assert len(set(pairs)) == 992 and {b for b, _ in pairs} == set(ab.INVALID)
    allowed = {name: set(int(x) for x in pos) for name, pos in regions}
    values, residues = defaultdict(set), defaultdict(set)
    for b, p, name in plan:
        assert p in allowed[name], (name, p)
        values[name].add(b)
        residues[name].add(p % 16)
    for name, pos in regions:
        assert values[name] == set(ab.INVALID), name
        assert residues[name] == {p % 16 for p in allowed[name]}, name  # every residue mod 16 the region has
        first, last = min(allowed[name]), max(allowed[name])
        assert {p for _, p, n in plan if n == name} & {first, first + 1, first + 2, first + 3}, name
        assert {p for _, p, n in plan if n == name} & {last, last - 1, last - 2, last - 3}, name


def test_every_batch_and_scan_path_of_the_gpu_file_has_a_full_plan():
    """the shapes of tests/test_gpu_alphabet.py: batch_legs' routing as the shape table states it, and a plan that covers each path's regions"""
    import test_gpu_alphabet as g
    region_sets = []
    for shape, (k, stride, count, off, out_off, kernels) in g.BATCH_SHAPES.items():
        got, regions = g.batch_regions(k, stride, count, off, out_off)
        assert got == kernels, shape
        region_sets.append((shape, regions))
    for off, from_skip, r992 in ((0, False, False), (3, False, True), (7, False, False), (9, True, False)):
        region_sets.append((f"scan+{off}", g.scan_regions(g._head(off) + g.SCAN_BODY, off, from_skip, r992=r992)))
    for name, regions in region_sets:
        plan = list(ab.reject_plan(regions))
        assert len({(b, p % 4) for b, p, _ in plan}) == 992, name
        for rname, pos in regions:
            assert {b for b, _, n in plan if n == rname} == set(ab.INVALID), (name, rname)
    kernels = " ".join(k for *_, k in g.BATCH_SHAPES.values())
    for k in ("kmer_dense_kernel", "kmer_slide2_kernel", "kmer_slide_any_kernel", "kmer_batch_kernel<true>", "kmer_batch_kernel<false>",
              *[f"kmer_slide_kernel<{s}>" for s in (1, 2, 4, 8, 16)]):
        assert k in kernels, k


def _search_specs():
    import alphabet_search as als
    for path, (make, make_gap) in als.PATHS.items():
        yield path, make(), False
        if make_gap:
            yield path, make_gap(), True  # (gap_fill asserts its own promise: every value before and behind an owned range at every byte lane)


def test_every_search_path_has_a_full_plan():
    """the paths of tests/test_gpu_alphabet_search.py: every region has a position at each byte lane, the regions partition the owned set, the
    plan's 992 cases reach every region with every value, owned and foreign positions are disjoint, and the input is valid where it is owned"""
    import alphabet_search as als
    names = set()
    for path, spec, is_gap in _search_specs():
        assert spec.name not in names, spec.name
        names.add(spec.name)
        owned = spec.owned
        assert owned.size and np.all(np.diff(owned) > 0) and owned[0] >= 0 and owned[-1] < spec.good.size, path
        assert 1 <= len(spec.regions) <= 4, path
        for rname, pos in spec.regions:
            assert {int(p) % 4 for p in pos} == {0, 1, 2, 3}, (path, rname)
        cat = np.concatenate([pos for _, pos in spec.regions])
        assert cat.size == owned.size and np.array_equal(np.sort(cat), owned), path  # a partition: nothing twice, nothing left out
        foreign = np.asarray(spec.foreign)
        assert not np.intersect1d(foreign, owned).size and len(set(spec.foreign)) == foreign.size, path
        assert foreign.min() == -16 and foreign.max() == spec.good.size + 31, path  # inside the Src's 256-byte pads
        assert np.array_equal(np.sort(np.concatenate([foreign[(foreign >= 0) & (foreign < spec.good.size)], owned])), np.arange(spec.good.size)), path
        assert np.isin(spec.unpolluted[owned], als.VALID).all() and np.array_equal(spec.good[owned], spec.unpolluted[owned]), path
        if is_gap:
            assert set(spec.good[foreign[(foreign >= 0) & (foreign < spec.good.size)]].tolist()) == set(range(256)), path
            continue
        plan = list(ab.reject_plan(spec.regions))
        assert len(plan) == 992 and len({(b, p % 4) for b, p, _ in plan}) == 992, path
        own = set(owned.tolist())
        for rname, pos in spec.regions:
            assert {b for b, _, n in plan if n == rname} == set(ab.INVALID), (path, rname)
        assert all(p in own for _, p, _ in plan), path


def test_search_paths_cover_the_entry_points_and_their_expected_values_see_only_owned_bytes(oracle):
    """every entry point the GPU file promises has a path; want() reports the first invalid OWNED byte and ignores the foreign ones"""
    import alphabet_search as als
    fns = {spec.name.split()[0] for _, spec, _ in _search_specs()}
    assert fns == {"kmer_hdist_best_async", "kmer_hdist_hist_async", "kmer_pattern_hits_async", "kmer_pattern_count_multi_async", "kmer_edist_best_async",
                   "kmer_edist_count_multi_async", "kmer_edist_hits_async", "reads_hdist_best_async", "reads_hdist_best2_async",
                   "reads_hdist_best_batch_async", "reads_hdist_anchored_async", "reads_hdist_anchored_batch_async", "reads_edist_anchored_async",
                   "reads_edist_anchored_batch_async", "reads_pattern_anchored_async", "reads_edist_best_async", "reads_edist_best_batch_async",
                   "reads_pattern_edist_best_async"}
    for path in ("reads_edist_anchored_batch-end", "reads_edist_best_batch", "reads_hdist_anchored-span19", "kmer_edist_hits-cap-below-dist-ref+5"):
        spec = als.PATHS[path][0]()
        want = spec.want(oracle, spec.good)
        assert [w.nbytes for w in want] == [nbytes for nbytes, _ in spec.outs][:len(want)] or "hits" in path
        inside = [p for p in spec.foreign if 0 <= p < spec.good.size]
        s = spec.good.copy()
        s[inside] = ord("N")
        assert all(np.array_equal(a, b) for a, b in zip(want, spec.want(oracle, s))), path
        a, b = int(spec.owned[spec.owned.size // 3]), int(spec.owned[-1])
        s[a], s[b] = ord("n"), 0
        with pytest.raises(oracle.OracleError) as ei:
            spec.want(oracle, s)
        assert (ei.value.kind, ei.value.byte, ei.value.index) == ("InvalidBase", ord("n"), a), path


def test_reject_plan_refuses_what_it_cannot_cover():
    with pytest.raises(ValueError):
        list(ab.reject_plan([(str(i), range(16 * i, 16 * i + 16)) for i in range(5)]))
    with pytest.raises(ValueError):
        list(ab.reject_plan([("head", range(0, 3)), ("body", range(3, 500))]))  # no position at lane 3
    with pytest.raises(ValueError):
        list(ab.reject_plan([]))


def test_recase_keeps_the_bases():
    rng = np.random.default_rng(3)
    s = ab.bases(rng, 500)
    assert set(s.tolist()) <= set(ab.VALID)
    for case in ("upper", "lower", "mixed"):
        t = ab.recase(s, case, 9)
        assert np.array_equal(t & 0xDF, s & 0xDF)
    assert set(ab.recase(s, "upper").tolist()) <= set(b"ACGT") and set(ab.recase(s, "lower").tolist()) <= set(b"acgt")
    both = set(ab.recase(s, "mixed", 9).tolist())
    assert both & set(b"ACGT") and both & set(b"acgt")
