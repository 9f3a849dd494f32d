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
