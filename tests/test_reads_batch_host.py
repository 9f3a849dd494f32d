"""CPU tests of the best match per read of a ragged batch (bitnuc_reads_hdist_best_batch / _batch_packed): the host path below the cutoff, through a
NULL context, against tests/reads_batch_oracle.py -- every k over lengths that include 0, k - 1, k and k + 1, ASCII and packed forms (junk in the pad
bits), equality with the fixed-length host forms on equal lengths, the tie rule, the fill values, every numbered argument check with its error kind
and value in the stated order, the table validation, INVALID_BASE with the absolute index (also inside a read shorter than k) leaving the outputs
untouched, and the host helpers (csrc/reads_batch_host.h) under ASan + UBSan in a stand-alone program (tests/c/reads_batch_host_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_batch_oracle as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = rb.NO_U32


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


def _p(a, byte_off=0):
    return C.c_void_p(a.ctypes.data + byte_off)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_batch_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads batch host ok" in out.stdout


@pytest.mark.parametrize("k", range(1, 33))
def test_host_path_every_k_lengths_around_k_and_query_count(k):
    free = _free()
    rng = np.random.default_rng(0xBA7C + k)
    pool = np.array([0, k - 1, k, k + 1, 31, 32, 33, 64, 150])
    for count in (1, 2, 9, 40):
        for nq in (1, 2, 17):
            lengths = pool[rng.integers(0, pool.size, size=count)]
            if count == 9:
                lengths[:4] = (0, k - 1, k, k + 1)
            queries = rb.random_queries(rng, nq, k)
            s, off = rb.random_batch(rng, lengths, k, queries)
            want = rb.batch_best(s, off, k, queries)
            got = free.reads_hdist_best_batch(s, off, k, queries)
            assert _same(got, want), ("ascii", k, list(lengths), nq)
            woff = rb.word_offsets_of(off)
            words = rb.pack_batch(s, off, seed=k)  # junk above every read's last base
            gotp = free.reads_hdist_best_batch_packed(words, woff, off, k, queries)
            assert _same(gotp, want), ("packed", k, list(lengths), nq)
            short = lengths < k
            assert (want[0][short] == NO).all() and (want[1][short] == NO).all() and (want[2][short] == 0xFF).all()
            assert (want[2][~short] != 0xFF).all()
            assert _same(rb.batch_best_by_scan(rb.numpy_scan, s, off, k, queries), want)  # the two oracles agree


@pytest.mark.parametrize("read_len", (1, 20, 31, 32, 33, 150))
def test_equal_lengths_give_the_fixed_length_answers(read_len):
    import reads_best_oracle as ro
    free = _free()
    rng = np.random.default_rng(700 + read_len)
    count = 12
    for k in (1, min(read_len, 7), min(read_len, 32)):
        queries = rb.random_queries(rng, 5, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        off = rb.offsets_of([read_len] * count)
        fixed = free.reads_hdist_best(s, read_len, k, queries)
        assert _same(free.reads_hdist_best_batch(s, off, k, queries), fixed)
        words = ro.pack_reads(s, read_len, count)  # encode_fixed's layout IS the ragged layout of equal lengths
        assert _same(free.reads_hdist_best_batch_packed(words, rb.word_offsets_of(off), off, k, queries), fixed)
        assert _same(free.reads_hdist_best_packed(words, read_len, count, k, queries), fixed)


def test_ties_lowest_query_then_lowest_offset_and_no_straddling():
    free = _free()
    rng = np.random.default_rng(34)
    k = 20
    lengths = [150, 0, 97, 200, 19, 60, 45]
    queries = rb.random_queries(rng, 24, k)
    queries[20] = queries[3]  # duplicate queries at indices 3 and 20
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    qc = rb.query_codes(queries[3], k)
    b3 = int(off[3])
    for p in (120, 17):  # two exact copies in read 3
        codes[b3 + p:b3 + p + k] = qc
    q9 = rb.query_codes(queries[9], k)
    b5 = int(off[5])
    codes[b5 - 7:b5 - 7 + k] = q9  # query 9 across the boundary of reads 4 and 5: seen by neither
    s = rb.LUT[codes].astype(np.uint8)
    want = rb.batch_best(s, off, k, queries)
    assert (int(want[0][3]), int(want[1][3]), int(want[2][3])) == (3, 17, 0)
    assert int(want[2][5]) > 0 and int(want[2][4]) == 0xFF and int(want[2][1]) == 0xFF
    pad = {4: list(q9[7:])}  # the packed form's pad bits of read 4 hold the bases that would complete the straddling match
    words = rb.pack_batch(s, off, pad_codes=pad)
    for got in (free.reads_hdist_best_batch(s, off, k, queries), free.reads_hdist_best_batch_packed(words, rb.word_offsets_of(off), off, k, queries)):
        assert _same(got, want)


def test_scalar_query_is_one_query():
    free = _free()
    rng = np.random.default_rng(6)
    queries = rb.random_queries(rng, 4, 12)
    s, off = rb.random_batch(rng, [80, 3, 50, 12, 0, 33], 12, queries)
    want = rb.batch_best(s, off, 12, queries[2:3])
    got = free.reads_hdist_best_batch(s, off, 12, int(queries[2]))
    assert _same(got, want) and (got[0][want[2] != 0xFF] == 0).all()


def test_no_window_fill_values():
    free = _free()
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    off = rb.offsets_of([6, 6, 6])
    woff = rb.word_offsets_of(off)
    w = np.zeros(3, dtype=np.uint64)
    for k, queries in ((0, [1, 2]), (19, [1, 2]), (3, [])):  # k == 0, total_bases < k, no queries
        for got in (free.reads_hdist_best_batch(s, off, k, queries), free.reads_hdist_best_batch_packed(w, woff, off, k, queries)):
            assert all(a.size == 3 for a in got)
            assert (got[0] == NO).all() and (got[1] == NO).all() and (got[2] == 0xFF).all()
    got = free.reads_hdist_best_batch(s, off, 7, [1, 2])  # total_bases >= k but no read holds a window
    assert (got[0] == NO).all() and (got[1] == NO).all() and (got[2] == 0xFF).all()
    empty = np.zeros(5, dtype=np.uint64)  # a batch of only empty reads
    for got in (free.reads_hdist_best_batch(s[:0], empty, 3, [1]), free.reads_hdist_best_batch_packed(w[:0], empty, empty, 3, [1])):
        assert all(a.size == 4 for a in got) and (got[2] == 0xFF).all()


def test_invalid_base_absolute_index_outputs_untouched():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    lengths = [50, 3, 0, 47, 5, 80]
    off = rb.offsets_of(lengths)
    s = np.frombuffer((b"ACGTACGTAC" * 20)[:int(off[-1])], dtype=np.uint8).copy()
    at = int(off[4]) + 2  # inside a read shorter than k
    s[at] = ord("N")
    s[int(off[5]) + 9] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_hdist_best_batch(s, off, 7, [0, 5, 9])
    assert (ei.value.byte, ei.value.index) == (ord("N"), at)
    q = np.zeros(3, dtype=np.uint64)
    bq = np.full(7, 0xAB, dtype=np.uint32)
    bp = np.full(7, 0xAB, dtype=np.uint32)
    bd = np.full(7, 0xAB, dtype=np.uint8)
    st, e = _raw(L.load().bitnuc_reads_hdist_best_batch, None, _p(s), _p(off), 6, 7, _p(q), 3, _p(bq), _p(bp), _p(bd))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), at)
    assert (bq == 0xAB).all() and (bp == 0xAB).all() and (bd == 0xAB).all()
    s[at] = ord("a")
    s[-1] = ord("-")  # the last byte of the batch
    st, e = _raw(L.load().bitnuc_reads_hdist_best_batch, None, _p(s), _p(off), 6, 7, _p(q), 3, _p(bq), _p(bp), _p(bd))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("x"), int(off[5]) + 9)


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_reads_hdist_best_batch, lib.bitnuc_reads_hdist_best_batch_packed
    adev, pdev = lib.bitnuc_reads_hdist_best_batch_async, lib.bitnuc_reads_hdist_best_batch_packed_async
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    words = np.zeros(9, dtype=np.uint64)
    off = rb.offsets_of([64, 64, 64, 64])
    woff = rb.word_offsets_of(off)
    q = np.zeros(8, dtype=np.uint64)
    bq = np.full(10, 0xAB, dtype=np.uint32)
    bp = np.full(10, 0xAB, dtype=np.uint32)
    bd = np.full(16, 0xAB, dtype=np.uint8)
    sp, wp, op, wop, qp, qo, po, do = _p(s), _p(words), _p(off), _p(woff), _p(q), _p(bq), _p(bp), _p(bd)

    def host(fn, src, o, wo, count, k, qq, nq, a, b, d):
        """both host forms through one argument list: the ASCII form has no word_offsets"""
        return _raw(fn, None, src, o, count, k, qq, nq, a, b, d) if fn is best else _raw(fn, None, src, wo, o, count, k, qq, nq, a, b, d)
    both = (best, packed)
    # 1. the _async forms check the context first, whatever else is wrong
    st, e = _raw(adev, None, None, None, 2**40, 2**60, 40, None, 70000, None, None, None)
    assert st == L.UNSUPPORTED and e.value == 0
    st, e = _raw(pdev, None, None, None, None, 2**40, 2**60, 40, None, 70000, None, None, None)
    assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with too many queries and NULL pointers everywhere
    for fn in both:
        st, e = host(fn, None, None, None, 2**40, 33, None, 70000, None, None, None)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 4. too many queries -> Unsupported with the count, before count == 0 and the array checks
    for fn in both:
        st, e = host(fn, None, None, None, 0, 5, None, 65537, None, None, None)
        assert st == L.UNSUPPORTED and e.value == 65537
    # 5. count == 0: OK, nothing written, even with NULL arrays and tables
    for fn in both:
        st, e = host(fn, None, None, None, 0, 5, None, 3, None, None, None)
        assert st == L.OK
    # 6. an output NULL, best_query / best_pos misaligned, queries NULL (with queries) or misaligned, a table NULL or misaligned -> Unsupported,
    # before the tables are read (they decrease here) and before the no-window case
    dec = np.array([0, 9, 5, 20, 30], dtype=np.uint64)
    dp = _p(dec)
    bad = ((None, qo, po, do), (qp, None, po, do), (qp, qo, None, do), (qp, qo, po, None), (_p(q, 4), qo, po, do), (qp, _p(bq, 2), po, do),
           (qp, qo, _p(bp, 1), do))
    for qq, a, b, d in bad:
        for fn, src in ((best, sp), (packed, wp)):
            st, e = host(fn, src, dp, dp, 4, 5, qq, 2, a, b, d)
            assert st == L.UNSUPPORTED and e.value == 0
    off9 = np.zeros(6, dtype=np.uint64)
    for o, wo in ((None, wop), (_p(off9, 4), wop)):
        for fn, src in ((best, sp), (packed, wp)):
            st, e = host(fn, src, o, wo, 4, 5, qp, 2, qo, po, do)
            assert st == L.UNSUPPORTED and e.value == 0
    for wo in (None, _p(off9, 4)):
        st, e = host(packed, wp, op, wo, 4, 5, qp, 2, qo, po, do)
        assert st == L.UNSUPPORTED and e.value == 0
    # 7. the tables, before the no-window case (k == 0 here) and before the data pointer (NULL here): decreasing offsets as encode_batch reports
    # them (value = the entry that decreased; the two are held against each other on a context in tests/test_gpu_reads_batch.py), offsets[0] != 0, word_offsets that are not encode_batch's, a read of 2^32 - 1 bases
    for fn in both:
        st, e = host(fn, None, dp, wop, 4, 0, qp, 2, qo, po, do)
        assert st == L.INVALID_RANGE and e.value == 2
        based = off + np.uint64(8)
        st, e = host(fn, None, _p(based), wop, 4, 0, qp, 2, qo, po, do)
        assert st == L.INVALID_RANGE and e.value == 0
        big = np.array([0, 10, 10 + 2**32 - 1], dtype=np.uint64)
        st, e = host(fn, None, _p(big), _p(rb.word_offsets_of(big)), 2, 0, qp, 2, qo, po, do)
        assert st == L.UNSUPPORTED and e.value == 2**32 - 1
    wrong = woff.copy()
    wrong[2] += np.uint64(1)
    st, e = host(packed, None, op, _p(wrong), 4, 0, qp, 2, qo, po, do)
    assert st == L.INVALID_RANGE and e.value == 2
    shifted = woff + np.uint64(1)
    st, e = host(packed, None, op, _p(shifted), 4, 0, qp, 2, qo, po, do)
    assert st == L.INVALID_RANGE and e.value == 0
    assert (bq == 0xAB).all() and (bp == 0xAB).all() and (bd == 0xAB).all()
    # 8. no windows: the fill values in [0, count) and nothing after, before the data pointer is looked at (NULL); dist at an odd address
    d1 = _p(bd, 1)
    short = rb.offsets_of([1, 2, 0, 1])
    for k, o, nq, qq in ((0, off, 8, qp), (5, short, 8, qp), (5, off, 0, None)):
        for fn in both:
            bq[:], bp[:], bd[:] = 0xAB, 0xAB, 0xAB
            st, _ = host(fn, None, _p(o), _p(rb.word_offsets_of(o)), 4, k, qq, nq, qo, po, d1)
            assert st == L.OK and (bq[:4] == NO).all() and (bq[4:] == 0xAB).all() and (bp[:4] == NO).all() and (bp[4:] == 0xAB).all()
            assert bd[0] == 0xAB and (bd[1:5] == 0xFF).all() and (bd[5:] == 0xAB).all()
    # 9. then NULL seq, or packed words NULL / not 8-byte aligned
    st, _ = host(best, None, op, wop, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    st, _ = host(packed, None, op, wop, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    st, _ = host(packed, _p(words, 4), op, wop, 4, 5, qp, 8, qo, po, do)
    assert st == L.UNSUPPORTED
    # and a valid call writes [0, count) of each output only
    bq[:], bp[:], bd[:] = 0xAB, 0xAB, 0xAB
    st, _ = host(best, sp, op, wop, 4, 5, qp, 3, qo, po, d1)
    assert st == L.OK and (bq[4:] == 0xAB).all() and (bp[4:] == 0xAB).all() and bd[0] == 0xAB and (bd[5:] == 0xAB).all()
    assert list(bq[:4]) == [0] * 4 and list(bp[:4]) == [0] * 4 and list(bd[1:5]) == [3] * 4  # AAAAA against ACGTACGT...: window 0 (ACGTA) differs in 3


def test_host_cutoff_is_judged_on_the_windows_of_the_reads_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported).  The windows are
    the sum over the reads of max(0, len - k + 1): reads shorter than k add bases and no windows."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    k = 16
    lengths = np.array([150, 9] * 700)  # 135 windows per long read: 94,500 in all; x 11 < 2^20 <= x 12
    off = rb.offsets_of(lengths)
    woff = rb.word_offsets_of(off)
    s = rb.LUT[np.random.default_rng(1).integers(0, 4, size=int(off[-1]))].astype(np.uint8)
    w = rb.pack_batch(s, off)
    count = lengths.size
    for nq, on_host in ((11, True), (12, False)):
        q = np.zeros(nq, dtype=np.uint64)
        bq, bp, bd = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint8)
        st, _ = _raw(lib.bitnuc_reads_hdist_best_batch, None, _p(s), _p(off), count, k, _p(q), nq, _p(bq), _p(bp), _p(bd))
        assert st == (L.OK if on_host else L.UNSUPPORTED), nq
        st, _ = _raw(lib.bitnuc_reads_hdist_best_batch_packed, None, _p(w), _p(woff), _p(off), count, k, _p(q), nq, _p(bq), _p(bp), _p(bd))
        assert st == (L.OK if on_host else L.UNSUPPORTED), nq


def test_the_async_forms_bound_their_totals_before_the_query_count():
    """check 3 of the _async forms (a total of 2^58 or more) needs a context to get past check 1: tests/test_gpu_reads_batch.py.  Here: the symbols are
    exported and declared (tests/test_abi.py compares the three declarations)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    for name in ("bitnuc_reads_hdist_best_batch_async", "bitnuc_reads_hdist_best_batch_packed_async", "bitnuc_reads_hdist_best_batch",
                 "bitnuc_reads_hdist_best_batch_packed"):
        assert hasattr(lib, name) and name in L.SIGNATURES
