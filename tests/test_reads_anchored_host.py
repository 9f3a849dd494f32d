"""CPU tests of the anchored best match and runner-up per read (bitnuc_reads_hdist_anchored / _anchored_packed): the host path below the cutoff, through a
NULL context, against tests/reads_anchored_oracle.py -- k in {1, 2, 16, 31, 32}; start, interior and 3' anchors; pos_hi clamped by the read's end; empty
ranges; span 64 accepted and span 65 Unsupported with value 65; the second triple as NULL pointers (the best triple equal to the six-output call's, the
guards intact) and one or two of them NULL -> Unsupported; every argument check in order with the guarded outputs untouched; an N inside the span
reported with its absolute index, an N outside ignored; the identity with reads_hdist_best2 at read_len <= 64; the cutoff judged on count x offsets x
queries; and the host helpers (csrc/reads_anchored_host.h) under ASan + UBSan in a stand-alone program (tests/c/reads_anchored_host_sanitize.cpp).
Every comparison is exact equality of all written arrays; guard words and bytes surround the six outputs, both dist arrays start at odd byte offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_anchored_oracle as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = ro.NO_U32
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
    """the six outputs inside guarded host buffers: GUARD words around query / pos, the dist arrays at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(4)]  # best_query, best_pos, second_query, second_pos
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
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        return w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy()


def _call(form, src, read_len, count, k, queries, pos_lo=0, pos_hi=None, second=True):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    fn = lib.bitnuc_reads_hdist_anchored if form == "ascii" else lib.bitnuc_reads_hdist_anchored_packed
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    o = Out(count)
    st, e = _raw(fn, None, C.c_void_p(src.ctypes.data) if src.size else None, read_len, count, k, pos_lo, SIZE_MAX if pos_hi is None else pos_hi,
                 C.c_void_p(q.ctypes.data) if q.size else None, q.size, *o.ptrs(second))
    return st, e, o


def _ranges(read_len, k):
    """(pos_lo, pos_hi) with a window and a span of at most 64: start, interior and 3' anchors, pos_hi clamped by the read's end"""
    last, most = read_len - k, 64 - k + 1
    out = set()
    for w in (1, 2, 4, most):
        w = min(w, last + 1)
        out |= {(0, w - 1), (last + 1 - w, None), ((last + 1 - w) // 2, (last + 1 - w) // 2 + w - 1), (last + 1 - w, last + 7), (last + 1 - w, SIZE_MAX - 1)}
    return sorted(out, key=lambda t: (t[0], -1 if t[1] is None else t[1]))


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_anchored_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads anchored host ok" in out.stdout


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_host_path_anchors_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0xA9C0 + k)
    for read_len in sorted({k, k + 1, 33, 64, 65, 150}):
        for pos_lo, pos_hi in _ranges(read_len, k):
            for count, nq in ((1, 1), (7, 2), (5, 17)):
                queries = ro.random_queries(rng, nq, k)
                s = ro.random_reads(rng, read_len, count, k, queries)
                want = ra.reads_anchored(s, read_len, count, k, queries, pos_lo, pos_hi)
                hi, span = ra.span_of(read_len, k, pos_lo, pos_hi)
                assert (want[1] >= pos_lo).all() and (want[1] <= hi).all()
                words = ro.pack_reads(s, read_len, count)  # junk above 2 * read_len in every read's last word
                for form, src in (("ascii", s), ("packed", words)):
                    st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_hi)
                    assert st == L.OK and _same(o.read(), want), (form, k, read_len, pos_lo, pos_hi, count, nq)
                    st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_hi, second=False)  # the best triple only
                    assert st == L.OK and _same(o.read()[:3], want[:3]) and o.untouched(which=(1,)), (form, k, read_len, pos_lo, pos_hi)
        queries = ro.random_queries(rng, 5, k)
        s = ro.random_reads(rng, read_len, 9, k, queries)
        lo = (read_len - k) // 2
        got = free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=lo + 1)  # the numpy wrappers
        assert _same(got, ra.reads_anchored(s, read_len, 9, k, queries, lo, lo + 1))
        assert _same(free.reads_hdist_anchored_packed(ro.pack_reads(s, read_len, 9), read_len, 9, k, queries, pos_lo=lo, pos_hi=lo + 1), got)
        assert _same(free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=lo + 1, second=False), got[:3])


@pytest.mark.parametrize("read_len", [1, 20, 33, 64])
def test_identity_with_best2_over_the_whole_read(read_len):
    free = _free()
    rng = np.random.default_rng(read_len)
    for k in sorted({1, 2, min(16, read_len), min(31, read_len), min(32, read_len)}):
        queries = ro.random_queries(rng, 9, k)
        s = ro.random_reads(rng, read_len, 11, k, queries)
        words = ro.pack_reads(s, read_len, 11)
        want = free.reads_hdist_best2(s, read_len, k, queries)
        assert _same(want, r2.reads_best2(s, read_len, 11, k, queries))
        assert _same(free.reads_hdist_anchored(s, read_len, k, queries), want)
        assert _same(free.reads_hdist_anchored_packed(words, read_len, 11, k, queries), free.reads_hdist_best2_packed(words, read_len, 11, k, queries))


def test_ties_the_range_is_honoured_and_the_winners_second_window_is_not_the_runner_up():
    free = _free()
    rng = np.random.default_rng(35)
    k, read_len, count, lo, hi = 20, 150, 6, 40, 75
    queries = ro.random_queries(rng, 24, k)
    queries[20] = queries[3] ^ (np.uint64(1) << np.uint64(63))  # an equal duplicate of query 3 at index 20 (junk above 2k differs)
    codes = rng.integers(0, 4, size=read_len * count)
    q3, q5, q12 = (ro.query_codes(queries[i], k) for i in (3, 5, 12))
    codes[2 * read_len + 45:2 * read_len + 45 + k] = q3  # read 2: query 3 (and its duplicate) exactly, inside the range
    near5 = q5.copy()
    near5[[2, 9]] ^= 1
    # reads 1 and 5: an exact copy of query 5 one base before / behind the range, a distance-2 copy inside
    codes[1 * read_len + lo - 1:1 * read_len + lo - 1 + k], codes[1 * read_len + 59:1 * read_len + 59 + k] = q5, near5
    codes[5 * read_len + hi + 1:5 * read_len + hi + 1 + k], codes[5 * read_len + 45:5 * read_len + 45 + k] = q5, near5
    near12 = q12.copy()
    near12[[3, 11]] ^= 3
    codes[4 * read_len + 41:4 * read_len + 41 + k] = near12  # read 4: query 12 with two changes
    s = ro.LUT[codes].astype(np.uint8)
    want = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    assert tuple(int(a[2]) for a in want) == (3, 45, 0, 20, 45, 0)
    assert tuple(int(a[1]) for a in want[:3]) == (5, 59, 2) and tuple(int(a[5]) for a in want[:3]) == (5, 45, 2)
    whole = r2.reads_best2(s, read_len, count, k, queries)  # the full-read search finds the copies outside
    assert tuple(int(a[1]) for a in whole[:3]) == (5, lo - 1, 0) and tuple(int(a[5]) for a in whole[:3]) == (5, hi + 1, 0)
    assert tuple(int(a[4]) for a in want[:3]) == (12, 41, 2)
    for got in (free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi),
                free.reads_hdist_anchored_packed(ro.pack_reads(s, read_len, count), read_len, count, k, queries, pos_lo=lo, pos_hi=hi)):
        assert _same(got, want)
    # a tie between two offsets of one query: the lower offset; the winner at two offsets and another query: the runner-up is the other query
    k, read_len = 8, 40
    queries = ro.random_queries(rng, 3, k)
    codes = rng.integers(0, 4, size=read_len)
    q1, q2 = ro.query_codes(queries[1], k), ro.query_codes(queries[2], k)
    one = q1.copy()
    one[4] ^= 1
    two = q2.copy()
    two[[0, 7]] ^= 2
    codes[3:3 + k], codes[12:12 + k], codes[22:22 + k], codes[31:31 + k] = q1, q1, one, two
    s = ro.LUT[codes].astype(np.uint8)
    got = free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=0, pos_hi=None)
    assert _same(got, ra.reads_anchored(s, read_len, 1, k, queries)) and tuple(int(a[0]) for a in got) == (1, 3, 0, 2, 31, 2)


def test_fills_empty_ranges_no_query_and_count_zero():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    w = np.zeros(3, dtype=np.uint64)
    for k, read_len, queries, pos_lo, pos_hi in ((0, 6, [1, 2], 0, None), (7, 6, [1, 2], 0, None), (3, 6, [], 0, None), (3, 6, [1, 2], 4, None), (3, 6, [1, 2], 2, 1),
                                                 (3, 6, [1, 2], SIZE_MAX, None), (3, 6, [1, 2], 9, 20)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, 3, k, queries, pos_lo, pos_hi)
            assert st == L.OK and _same(o.read(), r2.fill6(3)), (k, read_len, queries, pos_lo, pos_hi)
            assert _same(ra.reads_anchored(s, read_len, 3, k, queries, pos_lo, pos_hi), r2.fill6(3))
            st, _, o = _call(form, src, read_len, 3, k, queries, pos_lo, pos_hi, second=False)
            assert st == L.OK and _same(o.read()[:3], r2.fill6(3)[:3]) and o.untouched(which=(1,))
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
            want = ra.reads_anchored(s, read_len, count, k, queries, pos_lo, pos_lo + 64 - k)
            for form, src in (("ascii", s), ("packed", words)):
                st, _, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_lo + 64 - k)
                assert st == L.OK and _same(o.read(), want)
                if pos_lo + 65 <= read_len:
                    st, e, o = _call(form, src, read_len, count, k, queries, pos_lo, pos_lo + 65 - k)
                    assert st == L.UNSUPPORTED and e.value == 65 and o.untouched()
        for form, src in (("ascii", s), ("packed", words)):  # the whole read: span 150
            st, e, o = _call(form, src, read_len, count, k, queries)
            assert st == L.UNSUPPORTED and e.value == 150 and o.untouched()
            st, e, o = _call(form, src, read_len, count, k, [])  # the span is judged on (read_len, k, pos_lo, pos_hi) alone: also without queries
            assert st == L.UNSUPPORTED and e.value == 150 and o.untouched()
            st, e, o = _call(form, src, read_len, count, k, [], 0, 64 - k)  # a span of 64 without queries: the fill
            assert st == L.OK and _same(o.read(), r2.fill6(count))


def test_invalid_base_inside_the_span_absolute_index_outside_ignored():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(12)
    read_len, count, k, lo, hi = 50, 12, 7, 10, 13  # the span: bytes 10 .. 19 of every read
    queries = ro.random_queries(rng, 3, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    clean = ra.reads_anchored(s, read_len, count, k, queries, lo, hi)
    s[0 * read_len + 9] = ord("N")   # one base before read 0's span
    s[3 * read_len + 20] = ord("n")  # one base behind read 3's
    s[count * read_len - 1] = 0
    st, _, o = _call("ascii", s, read_len, count, k, queries, lo, hi)
    assert st == L.OK and _same(o.read(), clean)
    assert _same(free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi), clean)
    s[9 * read_len + 10] = ord("x")
    s[7 * read_len + 19] = ord("N")  # the last byte of read 7's span: the first invalid one in buffer order
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_hdist_anchored(s, read_len, k, queries, pos_lo=lo, pos_hi=hi)
    assert (ei.value.byte, ei.value.index) == (ord("N"), 7 * read_len + 19)
    st, e, o = _call("ascii", s, read_len, count, k, queries, lo, hi)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 7 * read_len + 19) and o.untouched()
    st, _, o = _call("ascii", s, read_len, count, k, queries, 30, 20)  # no window: nothing is read or validated
    assert st == L.OK and _same(o.read(), r2.fill6(count))


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_reads_hdist_anchored, lib.bitnuc_reads_hdist_anchored_packed
    adev, pdev = lib.bitnuc_reads_hdist_anchored_async, lib.bitnuc_reads_hdist_anchored_packed_async
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(9, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(8, dtype=np.uint64)
    qp = C.c_void_p(q.ctypes.data)
    o = Out(8)
    outs = o.ptrs()
    none6 = (None,) * 6
    both = (best, packed)
    # 1. the _async forms check the context first, whatever else is wrong
    for fn in (adev, pdev):
        st, e = _raw(fn, None, None, 2**40, 2**40, 40, 0, SIZE_MAX, None, 70000, *none6)
        assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with an impossible batch, too many queries, too wide a span and NULL pointers everywhere
    for fn in both:
        st, e = _raw(fn, None, None, 2**40, 2**40, 33, 0, SIZE_MAX, None, 70000, *none6)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. read_len >= 2^32 - 1, or count * read_len / count * wpr * 32 not below 2^58 -> Unsupported with read_len
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
    # 7. a best output NULL, one or two of the second outputs NULL, a query / pos array of either triple misaligned, queries NULL (with queries) or
    # misaligned -> Unsupported, before the no-window case (read_len 3 < k 5)
    def shifted(i, by):
        return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
    bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
    bad += [(qp, tuple(None if j in pair else p for j, p in enumerate(outs))) for pair in ((3, 4), (3, 5), (4, 5), (0, 3, 4, 5))]
    bad += [(None, outs), (C.c_void_p(q.ctypes.data + 4), outs)]
    bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1)), (qp, shifted(4, 2))]  # (4: second_pos)
    for qq, six in bad:
        for fn, src in ((best, sp), (packed, wp)):
            st, e = _raw(fn, None, src, 3, 4, 5, 0, SIZE_MAX, qq, 2, *six)
            assert st == L.UNSUPPORTED and e.value == 0
    assert o.untouched()
    # 8. no windows: the fill in [0, count) of all six and nothing after, before the reads are looked at (NULL); both dist arrays at odd addresses
    for k, read_len, nq, qq, lo in ((0, 100, 8, qp, 0), (6, 5, 8, qp, 0), (5, 100, 0, None, 0), (5, 100, 8, qp, 96)):
        for fn in both:
            o = Out(8)
            st, _ = _raw(fn, None, None, read_len, 8, k, lo, SIZE_MAX if lo else 3, qq, nq, *o.ptrs())
            assert st == L.OK and _same(o.read(), r2.fill6(8))
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
    # and a valid call writes [0, count) of each output only: AAAAA (queries 0 .. 2, equal) against ACGTACGT...: offset 1 (CGTAC) differs in 4,
    # offset 3 (TACGT) in 4, offset 2 (GTACG) in 4; offsets 1 .. 3 -> the lowest
    o = Out(4)
    st, _ = _raw(best, None, sp, 64, 4, 5, 1, 3, qp, 3, *o.ptrs())
    got = o.read()
    assert st == L.OK and [list(a) for a in got] == [[0] * 4, [1] * 4, [4] * 4, [1] * 4, [1] * 4, [4] * 4]


def test_host_cutoff_is_judged_on_count_times_offsets_times_queries():
    """Below the cutoff (1 Mi offsets x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    read_len, count, k = 150, 23625, 16  # four offsets per read: 94,500 in all; x 11 < 2^20 <= x 12
    s = ro.LUT[np.random.default_rng(1).integers(0, 4, size=read_len * count)].astype(np.uint8)
    w = ro.pack_reads(s, read_len, count)
    for nq, host in ((11, True), (12, False)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, count, k, np.arange(nq, dtype=np.uint64), read_len - k - 3, None)
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            if not host:
                assert o.untouched()
