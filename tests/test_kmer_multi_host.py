"""CPU tests of the multi-query k-mer count (bitnuc_kmer_hdist_count_multi / _multi_packed): the host path below the cutoff against the oracle's scan
per query, the argument checks and their order through api.context_free(), the host helpers (csrc/scan_multi_host.h) under ASan + UBSan
(tests/c/multi_host_sanitize.cpp), and an integer emulation of the ASCII three-channel contraction the count kernels run (tests/c/ascii_scan_emulate.cpp:
the (A, C) / G strip, count3_mfma_table, the row scales and the start values)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _run_harness(tmp_path, name, marker):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert marker in out.stdout


def test_host_helpers_under_asan_ubsan(tmp_path):
    _run_harness(tmp_path, "multi_host_sanitize", "multi host ok")


def test_ascii_contraction_emulated_under_asan_ubsan(tmp_path):
    """count3_mfma_table, row scales and start values applied to the strip expand3 builds from ASCII bytes: the threshold bits and the hit count are
    exact for every k in 1..32 and tau in {0, 1, k-1, k, k+1, 2^32-1}, with every partial sum below 2^24."""
    _run_harness(tmp_path, "ascii_scan_emulate", "ascii scan emulation ok")


def _want(oracle, s, k, queries, taus):
    if s.size < k or k == 0:
        return np.zeros(len(queries), dtype=np.uint64)
    return np.array([int(np.count_nonzero(oracle.kmer_hdist_scan(s, k, int(q)) <= int(t))) for q, t in zip(queries, taus)], dtype=np.uint64)


def test_host_path_every_k_against_the_oracle(oracle):
    free = _free()
    rng = np.random.default_rng(0x3117)
    lut = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    for k in range(1, 33):
        for nq in (1, 2, 33):
            for n in (k - 1, k, k + 1, 200, 1057):
                codes = rng.integers(0, 4, size=n)
                queries = rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2)  # junk above 2k
                if n >= k:
                    for i in range(0, nq, 2):  # every other query a window of the sequence
                        p = int(rng.integers(0, n - k + 1))
                        w = sum(int(c) << (2 * b) for b, c in enumerate(codes[p:p + k]))
                        queries[i] = np.uint64(w | ((int(queries[i]) << (2 * k)) & (2**64 - 1) if k < 32 else w))
                pool = [0, 1, max(k - 1, 0), k, 2**32 - 1]
                taus = np.array([pool[(i + n) % 5] for i in range(nq)], dtype=np.uint32)
                s = lut[codes + 4 * rng.integers(0, 2, size=n)].astype(np.uint8)
                want = _want(oracle, s, k, queries, taus)
                got = free.kmer_hdist_count_multi(s, k, queries, taus)
                assert got.dtype == np.uint64 and np.array_equal(got, want), (k, nq, n)
                words = oracle.encode(s) if n else np.zeros(0, dtype=np.uint64)
                assert np.array_equal(free.kmer_hdist_count_multi_packed(words, n, k, queries, taus), want), (k, nq, n)


def test_scalar_tau_broadcast_and_the_sequence_method(oracle):
    import bitnuc_amd as bn
    free = _free()
    rng = np.random.default_rng(4)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=3000)].copy()
    queries = rng.integers(0, 2**40, size=7, dtype=np.uint64)
    want = _want(oracle, s, 21, queries, [6] * 7)
    assert np.array_equal(free.kmer_hdist_count_multi(s, 21, queries, 6), want)
    assert np.array_equal(free.kmer_hdist_count_multi(s, 21, list(int(q) for q in queries), [6] * 7), want)
    ps = bn.PackedSequence.__new__(bn.PackedSequence)  # (its constructor encodes on the device: the fields by hand)
    ps.data, ps.length, ps._ctx = oracle.encode(s), s.size, free
    assert np.array_equal(ps.kmer_hdist_count_multi(21, queries, 6), want)
    with pytest.raises(ValueError):
        free.kmer_hdist_count_multi(s, 21, queries, [1, 2])


def test_mismatch_profile_in_one_call(oracle):
    free = _free()
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 4, size=5000)
    k = 20
    q = sum(int(c) << (2 * b) for b, c in enumerate(codes[100:100 + k]))
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].copy()
    d = oracle.kmer_hdist_scan(s, k, q)
    got = free.kmer_hdist_count_multi(s, k, [q] * 4, [0, 1, 2, 3])
    assert list(got) == [int(np.count_nonzero(d <= t)) for t in range(4)] and got[0] >= 1


def test_invalid_byte_on_the_host_path():
    import bitnuc_amd as bn
    free = _free()
    s = np.frombuffer(b"ACGTACGTAC" * 50, dtype=np.uint8).copy()
    s[123] = ord("N")
    s[400] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.kmer_hdist_count_multi(s, 7, [0, 5, 9], 3)
    assert (ei.value.byte, ei.value.index) == (ord("N"), 123)


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    multi, packed = lib.bitnuc_kmer_hdist_count_multi, lib.bitnuc_kmer_hdist_count_multi_packed
    mdev, pdev = lib.bitnuc_kmer_hdist_count_multi_dev, lib.bitnuc_kmer_hdist_count_multi_packed_dev
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(8, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(8, dtype=np.uint64)
    qp = C.c_void_p(q.ctypes.data)
    t = np.zeros(8, dtype=np.uint32)
    tp = C.c_void_p(t.ctypes.data)
    counts = np.full(10, 0xAB, dtype=np.uint64)
    cp = C.c_void_p(counts.ctypes.data)
    # 1. the _dev forms check the context first, whatever else is wrong
    st, e = _raw(mdev, None, None, 256, 40, None, None, 70000, None)
    assert st == L.UNSUPPORTED and e.value == 0
    st, e = _raw(pdev, None, None, 0, 100, 40, None, None, 70000, None)
    assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with NULL pointers everywhere and too many queries
    st, e = _raw(multi, None, None, 256, 33, None, None, 70000, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    st, e = _raw(packed, None, None, 0, 100, 33, None, None, 70000, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. packed: too few words for n -> InvalidLength(n), before the query checks
    st, e = _raw(packed, None, None, 3, 97, 5, None, None, 70000, None)
    assert st == L.INVALID_LENGTH and e.value == 97
    # 4. no queries: OK, nothing written, even with NULL arrays
    for fn, args in ((multi, (sp, 256, 5)), (packed, (wp, 8, 256, 5))):
        st, e = _raw(fn, None, *args, None, None, 0, None)
        assert st == L.OK
    # 5. too many queries -> Unsupported with the count, before the array checks
    st, e = _raw(multi, None, sp, 256, 5, None, None, 65537, None)
    assert st == L.UNSUPPORTED and e.value == 65537
    st, e = _raw(packed, None, wp, 8, 256, 5, None, None, 65537, None)
    assert st == L.UNSUPPORTED and e.value == 65537
    # 6. counts / queries / taus NULL or misaligned -> Unsupported, before the no-window case
    for qq, tt, cc in ((None, tp, cp), (qp, None, cp), (qp, tp, None), (C.c_void_p(q.ctypes.data + 4), tp, cp), (qp, C.c_void_p(t.ctypes.data + 2), cp),
                       (qp, tp, C.c_void_p(counts.ctypes.data + 4))):
        st, e = _raw(multi, None, sp, 3, 5, qq, tt, 2, cc)
        assert st == L.UNSUPPORTED and e.value == 0
        st, e = _raw(packed, None, wp, 8, 3, 5, qq, tt, 2, cc)
        assert st == L.UNSUPPORTED and e.value == 0
    # 7. no windows: every count 0 (and nothing after them), before the reference is looked at
    for k, n in ((0, 100), (6, 5)):
        counts[:] = 0xAB
        st, _ = _raw(multi, None, None, n, k, qp, tp, 8, cp)
        assert st == L.OK and (counts[:8] == 0).all() and (counts[8:] == 0xAB).all()
        counts[:] = 0xAB
        st, _ = _raw(packed, None, None, 8, n, k, qp, tp, 8, cp)
        assert st == L.OK and (counts[:8] == 0).all() and (counts[8:] == 0xAB).all()
    # 8. then a NULL reference, or packed words not 8-byte aligned
    st, _ = _raw(multi, None, None, 256, 5, qp, tp, 8, cp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, None, 8, 256, 5, qp, tp, 8, cp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 7, 200, 5, qp, tp, 8, cp)
    assert st == L.UNSUPPORTED
    # and a valid call writes counts[0 .. n_queries) only
    counts[:] = 0xAB
    st, _ = _raw(multi, None, sp, 256, 5, qp, tp, 3, cp)
    assert st == L.OK and (counts[3:] == 0xAB).all()


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=100_000)].copy()
    k = 16
    for nq, host in ((10, True), (11, False)):  # 99,985 windows: x 10 < 2^20 <= x 11
        q = np.zeros(nq, dtype=np.uint64)
        t = np.zeros(nq, dtype=np.uint32)
        counts = np.zeros(nq, dtype=np.uint64)
        st, _ = _raw(lib.bitnuc_kmer_hdist_count_multi, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data), nq,
                     C.c_void_p(counts.ctypes.data))
        assert st == (L.OK if host else L.UNSUPPORTED), nq
