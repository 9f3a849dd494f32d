"""CPU tests of the best match per query (bitnuc_kmer_hdist_best / _best_packed): the host path below the cutoff against the oracle's scan + argmin
per query, ties (the first position wins), the no-window fill, the argument checks and their order through a NULL context, invalid bytes, and the
host helpers (csrc/scan_best_host.h) with the device tables' row builders under ASan + UBSan (tests/c/best_host_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_POS = np.uint64(2**64 - 1)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "best_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "best host ok" in out.stdout


def _want(oracle, s, k, queries):
    """(pos, dist) by the oracle's scan and numpy's argmin / min (argmin returns the first minimum)"""
    nq = len(queries)
    if s.size < k or k == 0:
        return np.full(nq, NO_POS, dtype=np.uint64), np.full(nq, 0xFF, dtype=np.uint8)
    pos, dist = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint8)
    for i, q in enumerate(queries):
        d = oracle.kmer_hdist_scan(s, k, int(q))
        pos[i], dist[i] = np.argmin(d), np.min(d)
    return pos, dist


def test_host_path_every_k_against_the_oracle(oracle):
    free = _free()
    rng = np.random.default_rng(0xBE57)
    lut = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    for k in range(1, 33):
        for nq in (1, 2, 17):
            for n in (1, k - 1, k, k + 1, 33, 1057):
                codes = rng.integers(0, 4, size=n)
                queries = rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # junk above 2k
                if n >= k:
                    for i in range(0, nq, 2):  # every other query a window of the sequence, junk above 2k kept
                        p = int(rng.integers(0, n - k + 1))
                        w = sum(int(c) << (2 * b) for b, c in enumerate(codes[p:p + k]))
                        queries[i] = np.uint64(w if k == 32 else w | ((int(queries[i]) << (2 * k)) & (2**64 - 1)))
                s = lut[codes + 4 * rng.integers(0, 2, size=n)].astype(np.uint8)
                wpos, wdist = _want(oracle, s, k, queries)
                pos, dist = free.kmer_hdist_best(s, k, queries)
                assert pos.dtype == np.uint64 and dist.dtype == np.uint8
                assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist), (k, nq, n)
                words = oracle.encode(s) if n else np.zeros(0, dtype=np.uint64)
                if n % 32:
                    words = words.copy()
                    words[-1] |= np.uint64(0xDEADBEEFCAFEF00D) & ~np.uint64((1 << (2 * (n % 32))) - 1)  # junk above 2n
                pos, dist = free.kmer_hdist_best_packed(words, n, k, queries)
                assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist), (k, nq, n)


def test_ties_give_the_first_position(oracle):
    free = _free()
    rng = np.random.default_rng(21)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    k, n = 24, 3000
    codes = rng.integers(0, 4, size=n)
    qc = rng.integers(0, 4, size=k)
    near = qc.copy()
    near[5] ^= 1
    for p in (700, 2100):
        codes[p:p + k] = qc
    for p in (300, 1500):
        codes[p:p + k] = near
    q = sum(int(c) << (2 * b) for b, c in enumerate(qc))
    qn = sum(int(c) << (2 * b) for b, c in enumerate(near))
    s = lut[codes].copy()
    pos, dist = free.kmer_hdist_best(s, k, [q, qn])
    assert list(pos) == [700, 300] and list(dist) == [0, 0]
    assert all(np.array_equal(a, b) for a, b in zip((pos, dist), _want(oracle, s, k, [q, qn])))
    # without the exact copies of `near`, its best is one of the copies of q at distance 1: the first one
    codes[300:300 + k] = rng.integers(0, 4, size=k)
    codes[1500:1500 + k] = rng.integers(0, 4, size=k)
    s = lut[codes].copy()
    pos, dist = free.kmer_hdist_best_packed(oracle.encode(s), n, k, [qn])
    assert (int(pos[0]), int(dist[0])) == (700, 1)
    assert all(np.array_equal(a, b) for a, b in zip((pos, dist), _want(oracle, s, k, [qn])))


def test_scalar_query_and_the_sequence_method(oracle):
    import bitnuc_amd as bn
    free = _free()
    rng = np.random.default_rng(4)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=3000)].copy()
    queries = rng.integers(0, 2**40, size=7, dtype=np.uint64)
    wpos, wdist = _want(oracle, s, 20, queries)
    pos, dist = free.kmer_hdist_best(s, 20, int(queries[3]))  # a scalar query: Q = 1
    assert pos.shape == (1,) and (pos[0], dist[0]) == (wpos[3], wdist[3])
    ps = bn.PackedSequence.__new__(bn.PackedSequence)  # (its constructor encodes on the device: the fields by hand)
    ps.data, ps.length, ps._ctx = oracle.encode(s), s.size, free
    pos, dist = ps.kmer_hdist_best(20, queries)
    assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist)


def test_no_windows_fill():
    free = _free()
    s = np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()
    for k, n in ((0, 6), (7, 6), (3, 0)):
        for pos, dist in (free.kmer_hdist_best(s[:n], k, [1, 2, 3]), free.kmer_hdist_best_packed(np.zeros(1, dtype=np.uint64), n, k, [1, 2, 3])):
            assert (pos == NO_POS).all() and (dist == 0xFF).all() and pos.size == 3 and dist.size == 3


def test_invalid_byte_first_index_outputs_untouched():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    s = np.frombuffer(b"ACGTACGTAC" * 50, dtype=np.uint8).copy()
    s[123] = ord("N")
    s[400] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.kmer_hdist_best(s, 7, [0, 5, 9])
    assert (ei.value.byte, ei.value.index) == (ord("N"), 123)
    q = np.zeros(3, dtype=np.uint64)
    pos = np.full(4, 0xAB, dtype=np.uint64)
    dist = np.full(4, 0xAB, dtype=np.uint8)
    st, e = _raw(L.load().bitnuc_kmer_hdist_best, None, C.c_void_p(s.ctypes.data), s.size, 7, C.c_void_p(q.ctypes.data), 3, C.c_void_p(pos.ctypes.data),
                 C.c_void_p(dist.ctypes.data))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 123)
    assert (pos == 0xAB).all() and (dist == 0xAB).all()


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_kmer_hdist_best, lib.bitnuc_kmer_hdist_best_packed
    adev, pdev = lib.bitnuc_kmer_hdist_best_async, lib.bitnuc_kmer_hdist_best_packed_async
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(8, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(8, dtype=np.uint64)
    qp = C.c_void_p(q.ctypes.data)
    pos = np.full(10, 0xAB, dtype=np.uint64)
    pp = C.c_void_p(pos.ctypes.data)
    dist = np.full(16, 0xAB, dtype=np.uint8)
    dp = C.c_void_p(dist.ctypes.data)
    # 1. the _async forms check the context first, whatever else is wrong
    st, e = _raw(adev, None, None, 256, 40, None, 70000, None, None)
    assert st == L.UNSUPPORTED and e.value == 0
    st, e = _raw(pdev, None, None, 0, 100, 40, None, 70000, None, None)
    assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with NULL pointers everywhere and too many queries
    st, e = _raw(best, None, None, 256, 33, None, 70000, None, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    st, e = _raw(packed, None, None, 0, 100, 33, None, 70000, None, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. packed: too few words for n -> InvalidLength(n), before the query checks
    st, e = _raw(packed, None, None, 3, 97, 5, None, 70000, None, None)
    assert st == L.INVALID_LENGTH and e.value == 97
    # 4. no queries: OK, nothing written, even with NULL arrays
    for fn, args in ((best, (sp, 256, 5)), (packed, (wp, 8, 256, 5))):
        st, e = _raw(fn, None, *args, None, 0, None, None)
        assert st == L.OK
    # 5. too many queries -> Unsupported with the count, before the array checks
    st, e = _raw(best, None, sp, 256, 5, None, 65537, None, None)
    assert st == L.UNSUPPORTED and e.value == 65537
    st, e = _raw(packed, None, wp, 8, 256, 5, None, 65537, None, None)
    assert st == L.UNSUPPORTED and e.value == 65537
    # 6. pos / queries NULL or misaligned, dist NULL -> Unsupported, before the no-window case
    for qq, ps, ds in ((None, pp, dp), (qp, None, dp), (qp, pp, None), (C.c_void_p(q.ctypes.data + 4), pp, dp), (qp, C.c_void_p(pos.ctypes.data + 4), dp)):
        st, e = _raw(best, None, sp, 3, 5, qq, 2, ps, ds)
        assert st == L.UNSUPPORTED and e.value == 0
        st, e = _raw(packed, None, wp, 8, 3, 5, qq, 2, ps, ds)
        assert st == L.UNSUPPORTED and e.value == 0
    # 7. no windows: the fill values (and nothing after them), before the reference is looked at; dist at an odd address
    d1 = C.c_void_p(dist.ctypes.data + 1)
    for k, n in ((0, 100), (6, 5)):
        for fn, head in ((best, (None, n, k)), (packed, (None, 8, n, k))):
            pos[:] = 0xAB
            dist[:] = 0xAB
            st, _ = _raw(fn, None, *head, qp, 8, pp, d1)
            assert st == L.OK and (pos[:8] == NO_POS).all() and (pos[8:] == 0xAB).all()
            assert dist[0] == 0xAB and (dist[1:9] == 0xFF).all() and (dist[9:] == 0xAB).all()
    # 8. then a NULL reference, or packed words not 8-byte aligned
    st, _ = _raw(best, None, None, 256, 5, qp, 8, pp, dp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, None, 8, 256, 5, qp, 8, pp, dp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 7, 200, 5, qp, 8, pp, dp)
    assert st == L.UNSUPPORTED
    # and a valid call writes pos[0 .. n_queries) and dist[0 .. n_queries) only
    pos[:] = 0xAB
    dist[:] = 0xAB
    st, _ = _raw(best, None, sp, 256, 5, qp, 3, pp, d1)
    assert st == L.OK and (pos[3:] == 0xAB).all() and dist[0] == 0xAB and (dist[4:] == 0xAB).all()
    assert list(pos[:3]) == [0, 0, 0] and list(dist[1:4]) == [3, 3, 3]  # AAAAA against ACGTACGT...: window 0 (ACGTA) differs in 3, none in fewer


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=100_000)].copy()
    k = 16
    for nq, host in ((10, True), (11, False)):  # 99,985 windows: x 10 < 2^20 <= x 11
        q = np.zeros(nq, dtype=np.uint64)
        pos = np.zeros(nq, dtype=np.uint64)
        dist = np.zeros(nq, dtype=np.uint8)
        st, _ = _raw(lib.bitnuc_kmer_hdist_best, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_void_p(q.ctypes.data), nq, C.c_void_p(pos.ctypes.data),
                     C.c_void_p(dist.ctypes.data))
        assert st == (L.OK if host else L.UNSUPPORTED), nq
