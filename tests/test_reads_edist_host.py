"""CPU tests of the indel-tolerant anchored match per read (bitnuc_reads_edist_anchored / _packed and the pattern twins): the host path below the cutoff,
through a NULL context, against tests/reads_edist_oracle.py (the plain DP; the host path is the bit-parallel recurrence) -- k in 1 .. 32 with spans
around k, 32, 33 and 64; planted reads with one deletion, one insertion, one substitution and two mixed edits, (dist, end) asserted by hand; ties (two
ends, two queries, a duplicate); an all-N pattern, a pattern with an empty set, singleton patterns equal to the exact form; best_dist <= the Hamming
form's on every read; fills and count == 0; span 64 accepted, 65 Unsupported with its value; an invalid byte inside the span with its absolute index
and the outputs untouched, outside ignored; the argument checks in their documented order; the cutoff judged on count x n x n_queries; and the host
helpers (csrc/reads_edist_host.h) under ASan + UBSan in a stand-alone program (tests/c/reads_edist_host_sanitize.cpp).  Every comparison is exact
equality of all written arrays; guard words and bytes surround the six outputs, both dist arrays start at odd byte offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pattern_oracle as po
import reads_anchored_oracle as ra
import reads_best_oracle as ro
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
SIZE_MAX = C.c_size_t(-1).value


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


class Out:
    """the six outputs inside guarded host buffers: GUARD words around query / end, the dist arrays at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(4)]  # best_query, best_end, second_query, second_end
        self.d = [np.full(off + count + GUARD, 0x5A, dtype=np.uint8) for off in (1, 3)]

    def ptrs(self, second=True):
        w = [C.c_void_p(a.ctypes.data + 4 * GUARD) for a in self.w]
        d = [C.c_void_p(a.ctypes.data + off) for a, off in zip(self.d, (1, 3))]
        return (w[0], w[1], d[0], w[2], w[3], d[1]) if second else (w[0], w[1], d[0], None, None, None)

    def untouched(self, which=(0, 1)):
        return all((self.w[2 * j + i] == FILL32).all() for j in which for i in (0, 1)) and all((self.d[j] == 0x5A).all() for j in which)

    def read(self):
        n = self.count
        for a in self.w:
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / end written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        return w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy()


def _call(form, src, read_len, count, k, queries, pos_lo=0, pos_hi=None, second=True, pattern=False):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_anchored" + ("" if form == "ascii" else "_packed")
    q = rp.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    nq = q.shape[0]
    o = Out(count)
    st, e = _raw(getattr(lib, name), None, C.c_void_p(src.ctypes.data) if src.size else None, read_len, count, k, pos_lo, SIZE_MAX if pos_hi is None else pos_hi,
                 C.c_void_p(q.ctypes.data) if nq else None, nq, *o.ptrs(second))
    return st, e, o


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_edist_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads edist host ok" in out.stdout


@pytest.mark.parametrize("k0", [1, 9, 17, 25])
def test_host_path_against_the_dp(k0):
    """k = k0 .. k0 + 7 (1 .. 32 over the four cases); spans n in {k, k + 1, 31, 32, 33, 63, 64} where admissible; start, interior and 3' anchors"""
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0xED15 + k0)
    read_len = 150
    for k in range(k0, k0 + 8):
        for n in sorted({k, k + 1, 31, 32, 33, 63, 64}):
            if n < k:
                continue
            pos_lo, pos_hi = [(0, n - k), (37, 37 + n - k), (read_len - n, None)][(k + n) % 3]
            count, nq = [(1, 1), (7, 2), (5, 9)][(k + 2 * n) % 3]
            queries = ro.random_queries(rng, nq, k)
            s = ro.random_reads(rng, read_len, count, k, queries)
            for r in range(count):  # a copy of a query with up to 3 edits inside every span
                c = eo.plant(rng, ro.query_codes(queries[r % nq], k), int(rng.integers(0, 4)))[:n]
                at = r * read_len + pos_lo + int(rng.integers(0, n - len(c) + 1))
                s[at:at + len(c)] = _ascii(c)
            want = eo.reads_edist(s, read_len, count, k, queries, pos_lo, pos_hi)
            assert (want[1] > pos_lo).all() and (want[1] <= pos_lo + n).all() and (want[2] <= k).all()
            words = ro.pack_reads(s, read_len, count)  # junk above 2 * read_len in every read's last word
            for form, src in (("ascii", s), ("packed", words)):
                st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_hi)
                assert st == L.OK and _same(o.read(), want), (form, k, n, pos_lo, count, nq)
                st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_hi, second=False)  # the best triple only
                assert st == L.OK and _same(o.read()[:3], want[:3]) and o.untouched(which=(1,)), (form, k, n)
    free = _free()  # the numpy wrappers
    got = free.reads_edist_anchored(s, read_len, k, queries, pos_lo=pos_lo, pos_hi=pos_hi)
    assert _same(got, want)
    assert _same(free.reads_edist_anchored_packed(words, read_len, count, k, queries, pos_lo=pos_lo, pos_hi=pos_hi), want)
    assert _same(free.reads_edist_anchored(s, read_len, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, second=False), want[:3])


def test_planted_indels_by_hand():
    """(dist, end) of query 1 by hand: the planted copy starts at span base 4, that is read offset 14, so its end is 14 + its length; the Hamming form sees
    about half of the bases behind an indel differ"""
    from bitnuc_amd import _lib as L
    k, read_len, lo, n, s, queries = eo.planted_cases()
    count = 5
    want = eo.reads_edist(s, read_len, count, k, queries, lo, lo + n - k)
    assert list(want[0]) == [1] * count
    assert list(want[2]) == [1, 1, 1, 2, 0]
    assert list(want[1]) == [14 + 15, 14 + 17, 14 + 16, 14 + 16, 14 + 16]
    ham = ra.reads_anchored(s, read_len, count, k, queries, lo, lo + n - k)
    assert (ham[2][:2] > 4).all() and list(ham[2][2:]) == [1, ham[2][3], 0] and ham[2][3] > 2
    words = ro.pack_reads(s, read_len, count)
    for form, src in (("ascii", s), ("packed", words)):
        st, _, o = _call(form, src, read_len, count, k, queries, lo, lo + n - k)
        assert st == L.OK and _same(o.read(), want), form
        st, _, o = _call(form, src, read_len, count, k, rp.singletons(queries, k), lo, lo + n - k, pattern=True)
        assert st == L.OK and _same(o.read(), want), form


def test_ties_two_ends_two_queries_and_a_duplicate():
    free = _free()
    k, read_len = 6, 40
    q = np.array([0, 1, 2, 3, 1, 0])
    codes = np.full(read_len, 2)
    codes[5:11], codes[20:26] = q, q                                          # the same distance at two ends: the smaller end
    s = _ascii(codes)
    far = ro.word_of([3] * k)
    queries = np.array([far, ro.word_of(q), far, ro.word_of(q) | (1 << 40)], dtype=np.uint64)  # 3: an equal duplicate of 1 (junk above 2k differs)
    got = free.reads_edist_anchored(s, read_len, k, queries, pos_lo=0, pos_hi=None)
    assert _same(got, eo.reads_edist(s, read_len, 1, k, queries)) and tuple(int(a[0]) for a in got) == (1, 11, 0, 3, 11, 0)
    got = free.reads_edist_anchored(s, read_len, k, queries, pos_lo=8, pos_hi=None)  # only the second copy is whole inside the span
    assert tuple(int(a[0]) for a in got) == (1, 26, 0, 3, 26, 0)
    near = q.copy()
    near[2] = 0
    queries = np.array([ro.word_of(near), far, ro.word_of(near)], dtype=np.uint64)  # two queries at the same distance: the smaller index, the other second
    got = free.reads_edist_anchored(s, read_len, k, queries)
    assert _same(got, eo.reads_edist(s, read_len, 1, k, queries)) and tuple(int(a[0]) for a in got) == (0, 11, 1, 2, 11, 1)
    got = free.reads_edist_anchored(s, read_len, k, queries[:1])              # one query: the fill in the second triple
    assert tuple(int(a[0]) for a in got) == (0, 11, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF)


def test_patterns_all_n_empty_set_and_singletons():
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0x9A7)
    for k, read_len, lo, hi in ((1, 20, 3, 9), (12, 50, 7, 30), (32, 150, 86, None)):
        count = 9
        queries = ro.random_queries(rng, 5, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        words = ro.pack_reads(s, read_len, count)
        exact = free.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi)
        sing = rp.singletons(queries, k)
        assert _same(free.reads_pattern_edist_anchored(s, read_len, k, sing, pos_lo=lo, pos_hi=hi), exact)  # byte for byte the exact form
        assert _same(free.reads_pattern_edist_anchored_packed(words, read_len, count, k, sing, pos_lo=lo, pos_hi=hi), exact)
        all_n = po.from_iupac("N" * k)
        got = free.reads_pattern_edist_anchored(s, read_len, k, [all_n, sing[0]], pos_lo=lo, pos_hi=hi)
        assert (got[0] == 0).all() and (got[1] == lo + k).all() and (got[2] == 0).all()  # all-N: (0, pos_lo + k)
        sets = [po.random_sets(rng, k) for _ in range(4)]
        sets[2] = [set() if i == k // 2 else x for i, x in enumerate(sets[2])]  # an empty set never matches
        pats = rp.as_patterns([po.from_sets(x) for x in sets])
        want = eo.reads_pattern_edist(s, read_len, count, k, pats, lo, hi)
        for form, src in (("ascii", s), ("packed", words)):
            st, _, o = _call(form, src, read_len, count, k, pats, lo, hi, pattern=True)
            assert st == L.OK and _same(o.read(), want), (form, k)
        empty = rp.as_patterns([po.from_sets([set()] * k)])
        got = free.reads_pattern_edist_anchored(s, read_len, k, empty, pos_lo=lo, pos_hi=hi, second=False)
        assert _same(got, eo.reads_pattern_edist(s, read_len, count, k, empty, lo, hi)[:3]) and (got[2] == k).all() and (got[1] == lo + 1).all()


def test_never_above_the_hamming_form():
    free = _free()
    rng = np.random.default_rng(0xBEE)
    for k, read_len, lo, hi in ((16, 150, 130, None), (31, 150, 100, 119), (5, 64, 0, None)):
        count = 64
        queries = ro.random_queries(rng, 12, k)
        s = ro.random_reads(rng, read_len, count, k, queries, plant=12)
        e = free.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi)
        h = free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi)
        assert (e[2] <= h[2]).all() and _same(e, eo.reads_edist(s, read_len, count, k, queries, lo, hi))


def test_fills_empty_ranges_no_query_and_count_zero():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    w = np.zeros(3, dtype=np.uint64)
    for k, read_len, queries, pos_lo, pos_hi in ((0, 6, [1, 2], 0, None), (7, 6, [1, 2], 0, None), (3, 6, [], 0, None), (3, 6, [1, 2], 4, None), (3, 6, [1, 2], 2, 1),
                                                 (3, 6, [1, 2], SIZE_MAX, None), (3, 6, [1, 2], 9, 20)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, 3, k, queries, pos_lo, pos_hi)
            assert st == L.OK and _same(o.read(), eo.fill6(3)), (k, read_len, queries, pos_lo, pos_hi)
            assert _same(eo.reads_edist(s, read_len, 3, k, queries, pos_lo, pos_hi), eo.fill6(3))
            st, _, o = _call(form, src, read_len, 3, k, queries, pos_lo, pos_hi, second=False)
            assert st == L.OK and _same(o.read()[:3], eo.fill6(3)[:3]) and o.untouched(which=(1,))
    for form, src in (("ascii", s), ("packed", w)):
        st, _, o = _call(form, src, 6, 0, 3, [1, 2])  # count == 0: nothing written
        assert st == L.OK and o.untouched()


def test_span_64_is_accepted_and_65_is_unsupported_with_its_value():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(64)
    read_len, count = 150, 5
    for k in (1, 16, 32):
        queries = ro.random_queries(rng, 3, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        words = ro.pack_reads(s, read_len, count)
        for pos_lo in (0, 37, read_len - 64):
            want = eo.reads_edist(s, read_len, count, k, queries, pos_lo, pos_lo + 64 - k)
            for form, src in (("ascii", s), ("packed", words)):
                st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_lo + 64 - k)
                assert st == L.OK and _same(o.read(), want)
                if pos_lo + 65 <= read_len:
                    st, e, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_lo + 65 - k)
                    assert st == L.UNSUPPORTED and e.value == 65 and o.untouched()
        for form, src in (("ascii", s), ("packed", words)):  # the whole read: span 150
            st, e, o = _call(form, src, read_len, count, k, queries)
            assert st == L.UNSUPPORTED and e.value == 150 and o.untouched()
            st, e, o = _call(form, src, read_len, count, k, [])  # judged on (read_len, k, pos_lo, pos_hi) alone: also without queries
            assert st == L.UNSUPPORTED and e.value == 150 and o.untouched()
            st, e, o = _call(form, src, read_len, count, k, [], 0, 64 - k)  # a span of 64 without queries: the fill
            assert st == L.OK and _same(o.read(), eo.fill6(count))


def test_invalid_base_inside_the_span_absolute_index_outside_ignored():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(12)
    read_len, count, k, lo, hi = 50, 12, 7, 10, 13  # the span: bytes 10 .. 19 of every read
    queries = ro.random_queries(rng, 3, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    clean = eo.reads_edist(s, read_len, count, k, queries, lo, hi)
    s[0 * read_len + 9] = ord("N")   # one base before read 0's span
    s[3 * read_len + 20] = ord("n")  # one base behind read 3's
    s[count * read_len - 1] = 0
    st, _, o = _call("ascii", s, read_len, count, k, queries, lo, hi)
    assert st == L.OK and _same(o.read(), clean)
    assert _same(free.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi), clean)
    s[9 * read_len + 10] = ord("x")
    s[7 * read_len + 19] = ord("N")  # the last byte of read 7's span: the first invalid one in buffer order
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_edist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi)
    assert (ei.value.byte, ei.value.index) == (ord("N"), 7 * read_len + 19)
    for pattern, qq in ((False, queries), (True, rp.singletons(queries, k))):
        st, e, o = _call("ascii", s, read_len, count, k, qq, lo, hi, pattern=pattern)
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 7 * read_len + 19) and o.untouched()
    st, _, o = _call("ascii", s, read_len, count, k, queries, 30, 20)  # no span: nothing is read or validated
    assert st == L.OK and _same(o.read(), eo.fill6(count))


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(9, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(32, dtype=np.uint64)  # eight patterns as well (all sets empty)
    qp = C.c_void_p(q.ctypes.data)
    none6 = (None,) * 6
    for kind, qalign in (("", 4), ("pattern_", 2)):  # a pointer that breaks the kind's alignment: 8 bytes exact, 4 bytes patterns
        best, packed = getattr(lib, f"bitnuc_reads_{kind}edist_anchored"), getattr(lib, f"bitnuc_reads_{kind}edist_anchored_packed")
        adev, pdev = getattr(lib, f"bitnuc_reads_{kind}edist_anchored_async"), getattr(lib, f"bitnuc_reads_{kind}edist_anchored_packed_async")
        o = Out(8)
        outs = o.ptrs()
        both = (best, packed)
        # 1. the _async forms check the context first, whatever else is wrong
        for fn in (adev, pdev):
            st, e = _raw(fn, None, None, 2**40, 2**40, 40, 0, SIZE_MAX, None, 70000, *none6)
            assert st == L.UNSUPPORTED and e.value == 0
        # 2. k > 32, even with an impossible batch, too many queries, too wide a span and NULL pointers everywhere
        for fn in both:
            st, e = _raw(fn, None, None, 2**40, 2**40, 33, 0, SIZE_MAX, None, 70000, *none6)
            assert st == L.SEQUENCE_TOO_LONG and e.value == 33
        # 3. read_len >= 2^32 - 1, or count * wpr * 32 not below 2^58 -> Unsupported with read_len
        for read_len, count in ((2**32 - 1, 1), (2**33, 0), (2**28, 2**30), (33, 2**52)):
            for fn in both:
                st, e = _raw(fn, None, None, read_len, count, 5, 0, SIZE_MAX, None, 70000, *none6)
                assert st == L.UNSUPPORTED and e.value == read_len, (read_len, count)
        # 4. too many queries -> Unsupported with the count, before the span, count == 0 and the array checks
        for fn in both:
            st, e = _raw(fn, None, None, 100, 0, 5, 0, SIZE_MAX, None, 65537, *none6)
            assert st == L.UNSUPPORTED and e.value == 65537
        # 5. the span, before count == 0 and the array checks
        for fn in both:
            st, e = _raw(fn, None, None, 100, 0, 5, 10, 80, None, 3, *none6)
            assert st == L.UNSUPPORTED and e.value == 75
        # 6. count == 0: OK, nothing written, even with NULL arrays
        for fn in both:
            st, e = _raw(fn, None, None, 64, 0, 5, 0, 3, None, 3, *none6)
            assert st == L.OK
        # 7. a best output NULL, one or two of the second outputs NULL, a query / end array of either triple misaligned, queries NULL (with queries) or
        # misaligned -> Unsupported, before the no-span case (read_len 3 < k 5)
        def shifted(i, by):
            return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
        bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
        bad += [(qp, tuple(None if j in pair else p for j, p in enumerate(outs))) for pair in ((3, 4), (3, 5), (4, 5), (0, 3, 4, 5))]
        bad += [(None, outs), (C.c_void_p(q.ctypes.data + qalign), outs)]
        bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1)), (qp, shifted(4, 2))]  # (4: second_end)
        for qq, six in bad:
            for fn, src in ((best, sp), (packed, wp)):
                st, e = _raw(fn, None, src, 3, 4, 5, 0, SIZE_MAX, qq, 2, *six)
                assert st == L.UNSUPPORTED and e.value == 0
        assert o.untouched()
        # 8. no span: the fill in [0, count) of all six and nothing after, before the reads are looked at (NULL); both dist arrays at odd addresses
        for k, read_len, nq, qq, lo in ((0, 100, 8, qp, 0), (6, 5, 8, qp, 0), (5, 100, 0, None, 0), (5, 100, 8, qp, 96)):
            for fn in both:
                o = Out(8)
                st, _ = _raw(fn, None, None, read_len, 8, k, lo, SIZE_MAX if lo else 3, qq, nq, *o.ptrs())
                assert st == L.OK and _same(o.read(), eo.fill6(8))
        # 9. then NULL reads, or packed words NULL / not 8-byte aligned
        o = Out(8)
        outs = o.ptrs()
        st, _ = _raw(best, None, None, 64, 4, 5, 0, 3, qp, 8, *outs)
        assert st == L.UNSUPPORTED
        st, _ = _raw(packed, None, None, 64, 4, 5, 0, 3, qp, 8, *outs)
        assert st == L.UNSUPPORTED
        st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 64, 4, 5, 0, 3, qp, 8, *outs)
        assert st == L.UNSUPPORTED
        assert o.untouched()
    # and a valid call writes [0, count) of each output only: AAAAA (queries 0 .. 2, equal) against the span CGTACGT of ACGTACGT...: one A matches, so
    # the distance is 4, first reached at span base 4 (CGTA: four bases deleted from the query, or the like), end = 1 + 4
    o = Out(4)
    st, _ = _raw(lib.bitnuc_reads_edist_anchored, None, sp, 64, 4, 5, 1, 3, qp, 3, *o.ptrs())
    got = o.read()
    assert st == L.OK and _same(got, eo.reads_edist(s, 64, 4, 5, q[:3], 1, 3))
    assert [list(a) for a in got] == [[0] * 4, [5] * 4, [4] * 4, [1] * 4, [5] * 4, [4] * 4]


def test_host_cutoff_is_judged_on_count_times_span_times_queries():
    """Below the cutoff (1 Mi span bases x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    read_len, count, k = 150, 5000, 16  # four offsets: n = 19, 95,000 span bases in all; x 11 < 2^20 <= x 12
    s = ro.LUT[np.random.default_rng(1).integers(0, 4, size=read_len * count)].astype(np.uint8)
    w = ro.pack_reads(s, read_len, count)
    for nq, host in ((11, True), (12, False)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, count, k, np.arange(nq, dtype=np.uint64), read_len - k - 3, None)
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            if not host:
                assert o.untouched()
