"""CPU tests of the best match per read (bitnuc_reads_hdist_best / _best_packed): the host path below the cutoff, through a NULL context, against
tests/reads_best_oracle.py -- every k, read lengths around k and the word size, ASCII and packed forms (junk in the pad bits), the tie rule
(distance, then query, then offset), the fill values, every numbered argument check with its error kind and value, INVALID_BASE with the absolute
index, and the host helpers (csrc/reads_best_host.h) under ASan + UBSan in a stand-alone program (tests/c/reads_best_host_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_best_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = ro.NO_U32


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _same(got, want):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_best_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads best host ok" in out.stdout


@pytest.mark.parametrize("k", range(1, 33))
def test_host_path_every_k_read_length_count_and_query_count(k):
    free = _free()
    rng = np.random.default_rng(0x4EAD + k)
    for read_len in sorted({k - 1, k, k + 1, 31, 32, 33, 64, 150}):
        for count in (1, 2, 7):
            for nq in (1, 2, 17):
                queries = ro.random_queries(rng, nq, k)
                s = ro.random_reads(rng, read_len, count, k, queries)
                want = ro.reads_best(s, read_len, count, k, queries)
                got = free.reads_hdist_best(s, read_len, k, queries, count=count)
                assert _same(got, want), ("ascii", k, read_len, count, nq)
                words = ro.pack_reads(s, read_len, count)  # junk above 2 * read_len in every read's last word
                gotp = free.reads_hdist_best_packed(words, read_len, count, k, queries)
                assert _same(gotp, want), ("packed", k, read_len, count, nq)
                assert _same(got, gotp)
                if read_len < k:
                    assert (want[0] == NO).all() and (want[1] == NO).all() and (want[2] == 0xFF).all()


def test_ties_lowest_query_then_lowest_offset():
    free = _free()
    rng = np.random.default_rng(33)
    k, read_len, count = 20, 150, 6
    queries = ro.random_queries(rng, 24, k)
    queries[20] = queries[3]  # duplicate queries at indices 3 and 20
    codes = rng.integers(0, 4, size=read_len * count)
    qc = ro.query_codes(queries[3], k)
    for p in (90, 17):  # two exact copies in read 2
        codes[2 * read_len + p:2 * read_len + p + k] = qc
    codes[4 * read_len + 60:4 * read_len + 60 + k] = ro.query_codes(queries[9], k)  # read 4: query 9 exactly, later in the read
    near = qc.copy()
    near[7] ^= 2
    codes[4 * read_len + 5:4 * read_len + 5 + k] = near  # ... and query 3 with one change, earlier: the distance decides first
    s = ro.LUT[codes].astype(np.uint8)
    want = ro.reads_best(s, read_len, count, k, queries)
    assert (int(want[0][2]), int(want[1][2]), int(want[2][2])) == (3, 17, 0)
    assert (int(want[0][4]), int(want[1][4]), int(want[2][4])) == (9, 60, 0)
    for got in (free.reads_hdist_best(s, read_len, k, queries), free.reads_hdist_best_packed(ro.pack_reads(s, read_len, count), read_len, count, k, queries)):
        assert _same(got, want)


def test_scalar_query_is_one_query():
    free = _free()
    rng = np.random.default_rng(5)
    queries = ro.random_queries(rng, 4, 12)
    s = ro.random_reads(rng, 80, 9, 12, queries)
    want = ro.reads_best(s, 80, 9, 12, queries[2:3])
    got = free.reads_hdist_best(s, 80, 12, int(queries[2]))
    assert _same(got, want) and (got[0] == 0).all()


def test_no_window_fill_values():
    free = _free()
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    w = np.zeros(3, dtype=np.uint64)
    for k, read_len, queries in ((0, 6, [1, 2]), (7, 6, [1, 2]), (3, 6, [])):
        for got in (free.reads_hdist_best(s, read_len, k, queries, count=3), free.reads_hdist_best_packed(w, read_len, 3, k, queries)):
            assert all(a.size == 3 for a in got)
            assert (got[0] == NO).all() and (got[1] == NO).all() and (got[2] == 0xFF).all()


def test_invalid_base_absolute_index_outputs_untouched():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    s = np.frombuffer(b"ACGTACGTAC" * 60, dtype=np.uint8).copy()  # 12 reads of 50
    s[7 * 50 + 49] = ord("N")  # the last base of read 7
    s[9 * 50 + 3] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_hdist_best(s, 50, 7, [0, 5, 9])
    assert (ei.value.byte, ei.value.index) == (ord("N"), 7 * 50 + 49)
    q = np.zeros(3, dtype=np.uint64)
    bq = np.full(13, 0xAB, dtype=np.uint32)
    bp = np.full(13, 0xAB, dtype=np.uint32)
    bd = np.full(13, 0xAB, dtype=np.uint8)
    st, e = _raw(L.load().bitnuc_reads_hdist_best, None, C.c_void_p(s.ctypes.data), 50, 12, 7, C.c_void_p(q.ctypes.data), 3, C.c_void_p(bq.ctypes.data),
                 C.c_void_p(bp.ctypes.data), C.c_void_p(bd.ctypes.data))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 7 * 50 + 49)
    assert (bq == 0xAB).all() and (bp == 0xAB).all() and (bd == 0xAB).all()


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_reads_hdist_best, lib.bitnuc_reads_hdist_best_packed
    adev, pdev = lib.bitnuc_reads_hdist_best_async, lib.bitnuc_reads_hdist_best_packed_async
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(9, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(8, dtype=np.uint64)
    qp = C.c_void_p(q.ctypes.data)
    bq = np.full(10, 0xAB, dtype=np.uint32)
    bp = np.full(10, 0xAB, dtype=np.uint32)
    bd = np.full(16, 0xAB, dtype=np.uint8)
    qo, po, do = C.c_void_p(bq.ctypes.data), C.c_void_p(bp.ctypes.data), C.c_void_p(bd.ctypes.data)
    both = (best, packed)
    # 1. the _async forms check the context first, whatever else is wrong
    for fn in (adev, pdev):
        st, e = _raw(fn, None, None, 2**40, 2**40, 40, None, 70000, None, None, None)
        assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with an impossible batch, too many queries and NULL pointers everywhere
    for fn in both:
        st, e = _raw(fn, None, None, 2**40, 2**40, 33, None, 70000, None, None, None)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. read_len >= 2^32 - 1, or count * read_len / count * wpr * 32 not below 2^58 -> Unsupported with read_len
    for read_len, count in ((2**32 - 1, 1), (2**33, 0), (2**28, 2**30), (33, 2**52)):  # (33, 2^52): 33 * 2^52 < 2^58 <= 64 * 2^52, the packed period
        for fn in both:
            st, e = _raw(fn, None, None, read_len, count, 5, None, 70000, None, None, None)
            assert st == L.UNSUPPORTED and e.value == read_len, (read_len, count)
    # 4. too many queries -> Unsupported with the count, before count == 0 and the array checks
    for fn in both:
        st, e = _raw(fn, None, None, 64, 0, 5, None, 65537, None, None, None)
        assert st == L.UNSUPPORTED and e.value == 65537
    # 5. count == 0: OK, nothing written, even with NULL arrays
    for fn in both:
        st, e = _raw(fn, None, None, 64, 0, 5, None, 3, None, None, None)
        assert st == L.OK
    # 6. an output NULL, best_query / best_pos misaligned, queries NULL (with queries) or misaligned -> Unsupported, before the no-window case
    bad = ((None, qo, po, do), (qp, None, po, do), (qp, qo, None, do), (qp, qo, po, None), (C.c_void_p(q.ctypes.data + 4), qo, po, do),
           (qp, C.c_void_p(bq.ctypes.data + 2), po, do), (qp, qo, C.c_void_p(bp.ctypes.data + 1), do))
    for qq, a, b, d in bad:
        for fn, src in ((best, sp), (packed, wp)):
            st, e = _raw(fn, None, src, 3, 4, 5, qq, 2, a, b, d)
            assert st == L.UNSUPPORTED and e.value == 0
    assert (bq == 0xAB).all() and (bp == 0xAB).all() and (bd == 0xAB).all()
    # 7. no windows: the fill values in [0, count) and nothing after, before the reads are looked at (NULL); dist at an odd address
    d1 = C.c_void_p(bd.ctypes.data + 1)
    for k, read_len, nq, qq in ((0, 100, 8, qp), (6, 5, 8, qp), (5, 100, 0, None)):
        for fn in both:
            bq[:], bp[:], bd[:] = 0xAB, 0xAB, 0xAB
            st, _ = _raw(fn, None, None, read_len, 8, k, qq, nq, qo, po, d1)
            assert st == L.OK and (bq[:8] == NO).all() and (bq[8:] == 0xAB).all() and (bp[:8] == NO).all() and (bp[8:] == 0xAB).all()
            assert bd[0] == 0xAB and (bd[1:9] == 0xFF).all() and (bd[9:] == 0xAB).all()
    # 8. then NULL reads, or packed words NULL / not 8-byte aligned
    st, _ = _raw(best, None, None, 64, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, None, 64, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 64, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    # and a valid call writes [0, count) of each output only
    bq[:], bp[:], bd[:] = 0xAB, 0xAB, 0xAB
    st, _ = _raw(best, None, sp, 64, 4, 5, qp, 3, qo, po, d1)
    assert st == L.OK and (bq[4:] == 0xAB).all() and (bp[4:] == 0xAB).all() and bd[0] == 0xAB and (bd[5:] == 0xAB).all()
    assert list(bq[:4]) == [0] * 4 and list(bp[:4]) == [0] * 4 and list(bd[1:5]) == [3] * 4  # AAAAA against ACGTACGT...: window 0 (ACGTA) differs in 3


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    read_len, count, k = 150, 700, 16  # 135 windows per read: 94,500 in all; x 11 < 2^20 <= x 12
    s = ro.LUT[np.random.default_rng(1).integers(0, 4, size=read_len * count)].astype(np.uint8)
    w = ro.pack_reads(s, read_len, count)
    for nq, host in ((11, True), (12, False)):
        q = np.zeros(nq, dtype=np.uint64)
        bq, bp, bd = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint8)
        for fn, src in ((lib.bitnuc_reads_hdist_best, s), (lib.bitnuc_reads_hdist_best_packed, w)):
            st, _ = _raw(fn, None, C.c_void_p(src.ctypes.data), read_len, count, k, C.c_void_p(q.ctypes.data), nq, C.c_void_p(bq.ctypes.data),
                         C.c_void_p(bp.ctypes.data), C.c_void_p(bd.ctypes.data))
            assert st == (L.OK if host else L.UNSUPPORTED), nq
