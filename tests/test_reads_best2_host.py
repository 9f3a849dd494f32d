"""CPU tests of the best match and the runner-up per read (bitnuc_reads_hdist_best2 / _best2_packed): the host path below the cutoff, through a NULL
context, against tests/reads_best2_oracle.py -- every k over read lengths k, k + 1, 33 and 150 with 1, 2, 3 and 17 queries, ASCII and packed forms
(junk in the pad bits); the tie rules (an equal duplicate query is the runner-up at the same distance; the winner's own second window never is); the
fills (no window, no or one query, count == 0); INVALID_BASE with the absolute index and all six outputs untouched; the argument checks and their
order, a misaligned second_pos included; the cutoff judged on windows x queries; and the host helpers (csrc/reads_best2_host.h) under ASan + UBSan in
a stand-alone program (tests/c/reads_best2_host_sanitize.cpp).  Every comparison is exact equality of all six arrays; guard words and bytes surround
the six outputs and both dist arrays start at odd byte offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = ro.NO_U32
GUARD = 4
FILL32 = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _same(got, want):
    return len(got) == 6 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


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

    def ptrs(self):
        w = [C.c_void_p(a.ctypes.data + 4 * GUARD) for a in self.w]
        d = [C.c_void_p(a.ctypes.data + off) for a, off in zip(self.d, (1, 3))]
        return w[0], w[1], d[0], w[2], w[3], d[1]

    def untouched(self):
        return all((a == FILL32).all() for a in self.w) and all((a == 0x5A).all() for a in self.d)

    def read(self):
        n = self.count
        for a in self.w:
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        return w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy()


def _call(form, src, read_len, count, k, queries):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    fn = lib.bitnuc_reads_hdist_best2 if form == "ascii" else lib.bitnuc_reads_hdist_best2_packed
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    o = Out(count)
    st, e = _raw(fn, None, C.c_void_p(src.ctypes.data) if src.size else None, read_len, count, k, C.c_void_p(q.ctypes.data) if q.size else None, q.size, *o.ptrs())
    return st, e, o


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_best2_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads best2 host ok" in out.stdout


@pytest.mark.parametrize("k", range(1, 33))
def test_host_path_every_k_read_length_and_query_count(k):
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0xB352 + k)
    for read_len in sorted({k, k + 1, 33, 150}):
        if read_len < k:
            continue
        for count in (1, 7):
            for nq in (1, 2, 3, 17):
                queries = ro.random_queries(rng, nq, k)
                s = ro.random_reads(rng, read_len, count, k, queries)
                want = r2.reads_best2(s, read_len, count, k, queries)
                words = ro.pack_reads(s, read_len, count)  # junk above 2 * read_len in every read's last word
                for form, src in (("ascii", s), ("packed", words)):
                    st, _, o = _call(form, src, read_len, count, k, queries)
                    assert st == L.OK and _same(o.read(), want), (form, k, read_len, count, nq)
                assert _same(want[:3] + want[:3], ro.reads_best(s, read_len, count, k, queries) * 2)  # the first triple is the best match's
                if nq == 1:
                    assert (want[3] == NO).all() and (want[4] == NO).all() and (want[5] == 0xFF).all() and (want[2] != 0xFF).all()
        queries = ro.random_queries(rng, 5, k)
        s = ro.random_reads(rng, read_len, 9, k, queries)
        got = free.reads_hdist_best2(s, read_len, k, queries)  # the numpy wrappers
        assert _same(got, r2.reads_best2(s, read_len, 9, k, queries))
        assert _same(free.reads_hdist_best2_packed(ro.pack_reads(s, read_len, 9), read_len, 9, k, queries), got)
        assert _same(got[:3] + got[:3], free.reads_hdist_best(s, read_len, k, queries) * 2)


def test_ties_a_duplicate_query_is_the_runner_up_and_the_winners_second_window_is_not():
    free = _free()
    rng = np.random.default_rng(34)
    k, read_len, count = 20, 150, 6
    queries = ro.random_queries(rng, 24, k)
    queries[20] = queries[3] ^ (np.uint64(1) << np.uint64(63))  # an equal duplicate of query 3 at index 20 (junk above 2k differs)
    codes = rng.integers(0, 4, size=read_len * count)
    qc = ro.query_codes(queries[3], k)
    for p in (90, 17):  # read 2: two exact copies of query 3
        codes[2 * read_len + p:2 * read_len + p + k] = qc
    # read 4: query 9 exactly at 60, again with one change at 100 (its own second window: distance 1), query 12 with two changes at 5
    q9, q12 = ro.query_codes(queries[9], k), ro.query_codes(queries[12], k)
    near9, near12 = q9.copy(), q12.copy()
    near9[7] ^= 2
    near12[3] ^= 1
    near12[11] ^= 3
    codes[4 * read_len + 60:4 * read_len + 60 + k] = q9
    codes[4 * read_len + 100:4 * read_len + 100 + k] = near9
    codes[4 * read_len + 5:4 * read_len + 5 + k] = near12
    s = ro.LUT[codes].astype(np.uint8)
    want = r2.reads_best2(s, read_len, count, k, queries)
    assert tuple(int(a[2]) for a in want) == (3, 17, 0, 20, 17, 0)
    assert tuple(int(a[4]) for a in want) == (9, 60, 0, 12, 5, 2)
    for got in (free.reads_hdist_best2(s, read_len, k, queries), free.reads_hdist_best2_packed(ro.pack_reads(s, read_len, count), read_len, count, k, queries)):
        assert _same(got, want)


def test_scalar_query_is_one_query_and_the_runner_up_is_the_fill():
    free = _free()
    rng = np.random.default_rng(6)
    queries = ro.random_queries(rng, 4, 12)
    s = ro.random_reads(rng, 80, 9, 12, queries)
    want = r2.reads_best2(s, 80, 9, 12, queries[2:3])
    got = free.reads_hdist_best2(s, 80, 12, int(queries[2]))
    assert _same(got, want) and (got[0] == 0).all() and (got[2] != 0xFF).all()
    assert (got[3] == NO).all() and (got[4] == NO).all() and (got[5] == 0xFF).all()


def test_fills_no_window_no_query_and_count_zero():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    w = np.zeros(3, dtype=np.uint64)
    for k, read_len, queries in ((0, 6, [1, 2]), (7, 6, [1, 2]), (3, 6, [])):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, 3, k, queries)
            got = o.read()
            assert st == L.OK and _same(got, r2.fill6(3)), (k, read_len, queries)
    for form, src in (("ascii", s), ("packed", w)):
        st, _, o = _call(form, src, 6, 0, 3, [1, 2])  # count == 0: nothing written
        assert st == L.OK and o.untouched()


def test_invalid_base_absolute_index_all_six_outputs_untouched():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    s = np.frombuffer(b"ACGTACGTAC" * 60, dtype=np.uint8).copy()  # 12 reads of 50
    s[7 * 50 + 49] = ord("N")  # the last base of read 7
    s[9 * 50 + 3] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_hdist_best2(s, 50, 7, [0, 5, 9])
    assert (ei.value.byte, ei.value.index) == (ord("N"), 7 * 50 + 49)
    st, e, o = _call("ascii", s, 50, 12, 7, [0, 5, 9])
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 7 * 50 + 49)
    assert o.untouched()


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_reads_hdist_best2, lib.bitnuc_reads_hdist_best2_packed
    adev, pdev = lib.bitnuc_reads_hdist_best2_async, lib.bitnuc_reads_hdist_best2_packed_async
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
        st, e = _raw(fn, None, None, 2**40, 2**40, 40, None, 70000, *none6)
        assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with an impossible batch, too many queries and NULL pointers everywhere
    for fn in both:
        st, e = _raw(fn, None, None, 2**40, 2**40, 33, None, 70000, *none6)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. read_len >= 2^32 - 1, or count * read_len / count * wpr * 32 not below 2^58 -> Unsupported with read_len
    for read_len, count in ((2**32 - 1, 1), (2**33, 0), (2**28, 2**30), (33, 2**52)):
        for fn in both:
            st, e = _raw(fn, None, None, read_len, count, 5, None, 70000, *none6)
            assert st == L.UNSUPPORTED and e.value == read_len, (read_len, count)
    # 4. too many queries -> Unsupported with the count, before count == 0 and the array checks
    for fn in both:
        st, e = _raw(fn, None, None, 64, 0, 5, None, 65537, *none6)
        assert st == L.UNSUPPORTED and e.value == 65537
    # 5. count == 0: OK, nothing written, even with NULL arrays
    for fn in both:
        st, e = _raw(fn, None, None, 64, 0, 5, None, 3, *none6)
        assert st == L.OK
    # 6. any of the six outputs NULL, a query / pos array of either triple misaligned, queries NULL (with queries) or misaligned -> Unsupported, before
    # the no-window case (read_len 3 < k 5)
    def shifted(i, by):
        return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
    bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
    bad += [(None, outs), (C.c_void_p(q.ctypes.data + 4), outs)]
    bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1)), (qp, shifted(4, 2))]  # (4: second_pos)
    for qq, six in bad:
        for fn, src in ((best, sp), (packed, wp)):
            st, e = _raw(fn, None, src, 3, 4, 5, qq, 2, *six)
            assert st == L.UNSUPPORTED and e.value == 0
    assert o.untouched()
    # 7. no windows: the fill in [0, count) of all six and nothing after, before the reads are looked at (NULL); both dist arrays at odd addresses
    for k, read_len, nq, qq in ((0, 100, 8, qp), (6, 5, 8, qp), (5, 100, 0, None)):
        for fn in both:
            o = Out(8)
            st, _ = _raw(fn, None, None, read_len, 8, k, qq, nq, *o.ptrs())
            assert st == L.OK and _same(o.read(), r2.fill6(8))
    # 8. then NULL reads, or packed words NULL / not 8-byte aligned
    o = Out(8)
    outs = o.ptrs()
    st, _ = _raw(best, None, None, 64, 4, 5, qp, 8, *outs)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, None, 64, 4, 5, qp, 8, *outs)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 64, 4, 5, qp, 8, *outs)
    assert st == L.UNSUPPORTED
    assert o.untouched()
    # and a valid call writes [0, count) of each output only: AAAAA (queries 0 .. 2, equal) against ACGTACGT...: window 0 (ACGTA) differs in 3
    o = Out(4)
    st, _ = _raw(best, None, sp, 64, 4, 5, qp, 3, *o.ptrs())
    got = o.read()
    assert st == L.OK and [list(a) for a in got] == [[0] * 4, [0] * 4, [3] * 4, [1] * 4, [0] * 4, [3] * 4]


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    read_len, count, k = 150, 700, 16  # 135 windows per read: 94,500 in all; x 11 < 2^20 <= x 12
    s = ro.LUT[np.random.default_rng(1).integers(0, 4, size=read_len * count)].astype(np.uint8)
    w = ro.pack_reads(s, read_len, count)
    for nq, host in ((11, True), (12, False)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _call(form, src, read_len, count, k, np.arange(nq, dtype=np.uint64))
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            if not host:
                assert o.untouched()
