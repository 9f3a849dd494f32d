"""CPU tests of the k-mer hit lists (bitnuc_kmer_hdist_hits / _hits_packed): the host path below the cutoff against np.flatnonzero over the
oracle's scan, the cap contract, the argument checks and their order through api.context_free(), and the host helpers (csrc/scan_hits_host.h)
under ASan + UBSan (tests/c/hits_host_sanitize.cpp)."""
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


def _taus(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 2**32 - 1})


def test_host_helpers_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "hits_host_sanitize")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", "hits_host_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "hits host ok" in out.stdout


def test_host_path_every_k_against_the_oracle(oracle):
    free = _free()
    rng = np.random.default_rng(0x417)
    lut = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    for k in range(1, 33):
        for n in (0, k - 1, k, k + 1, 100, 1057, 3000):
            q = rng.integers(0, 4, size=k)
            query = int(sum(int(c) << (2 * i) for i, c in enumerate(q))) | ((5 << 2 * k) & (2**64 - 1) if k < 32 else 0)
            codes = np.resize(q, n) if n % 2 else rng.integers(0, 4, size=n)
            s = lut[codes + 4 * rng.integers(0, 2, size=n)].astype(np.uint8)
            want_d = oracle.kmer_hdist_scan(s, k, query) if n >= k else np.zeros(0, dtype=np.uint8)
            words = oracle.encode(s) if n else np.zeros(0, dtype=np.uint64)
            for tau in _taus(k):
                want = np.flatnonzero(want_d <= tau)
                p, d = free.kmer_hdist_hits(s, k, query, tau, with_dist=True)
                assert p.dtype == np.uint64 and np.array_equal(p, want) and np.array_equal(d, want_d[want]), (k, n, tau)
                p2, d2 = free.kmer_hdist_hits_packed(words, n, k, query, tau, with_dist=True)
                assert np.array_equal(p2, want) and np.array_equal(d2, want_d[want]), (k, n, tau)
                assert np.array_equal(free.kmer_hdist_hits(s, k, query, tau), want)


def test_invalid_byte_on_the_host_path():
    import bitnuc_amd as bn
    free = _free()
    s = np.frombuffer(b"ACGTACGTAC" * 50, dtype=np.uint8).copy()
    s[123] = ord("N")
    s[400] = ord("x")
    with pytest.raises(bn.NucleotideError) as ei:
        free.kmer_hdist_hits(s, 7, 0, 3)
    assert (ei.value.byte, ei.value.index) == (ord("N"), 123)


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def test_cap_contract_on_the_host_path():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGTTGCA" * 300, dtype=np.uint8).copy()
    k, tau, query = 8, 2, 0b0001101111100100  # as_2bit(b"ACGTTGCA"): the windows at every 8th base hit
    nh = C.c_uint64(0)
    st, _ = _raw(lib.bitnuc_kmer_hdist_hits, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_uint64(query), tau, None, None, 0, C.byref(nh))
    assert st == L.OK
    total = nh.value
    assert total > 2
    full_pos = np.zeros(total, dtype=np.uint64)
    st, _ = _raw(lib.bitnuc_kmer_hdist_hits, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_uint64(query), tau, C.c_void_p(full_pos.ctypes.data), None, total, C.byref(nh))
    assert st == L.OK and nh.value == total
    for cap in (0, 1, total - 1, total, total + 5):
        pos = np.full(cap + 8, 0xA5, dtype=np.uint64)
        d = np.full(cap + 8, 0xEE, dtype=np.uint8)
        st, _ = _raw(lib.bitnuc_kmer_hdist_hits, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_uint64(query), tau, C.c_void_p(pos.ctypes.data),
                     C.c_void_p(d.ctypes.data), cap, C.byref(nh))
        assert st == L.OK and nh.value == total
        m = min(cap, total)
        assert np.array_equal(pos[:m], full_pos[:m]) and (pos[cap:] == 0xA5).all() and (d[cap:] == 0xEE).all()


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    hits, packed = lib.bitnuc_kmer_hdist_hits, lib.bitnuc_kmer_hdist_hits_packed
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(8, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    pos = np.zeros(300, dtype=np.uint64)
    pp = C.c_void_p(pos.ctypes.data)
    nh = C.c_uint64(77)
    # 1. k > 32 first, even with NULL pointers everywhere
    st, e = _raw(hits, None, None, 256, 33, C.c_uint64(0), 3, None, None, 10, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    st, e = _raw(packed, None, None, 0, 100, 33, C.c_uint64(0), 3, None, None, 10, None)
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 2. packed: too few words for n -> InvalidLength(n), before the output checks
    st, e = _raw(packed, None, None, 3, 97, 5, C.c_uint64(0), 3, None, None, 10, None)
    assert st == L.INVALID_LENGTH and e.value == 97
    # 3. n_hits NULL, or pos NULL with cap > 0: Unsupported (before the no-window case)
    for fn, head in ((hits, (sp, 256)), (packed, (wp, 8, 256))):
        st, _ = _raw(fn, None, *head, 5, C.c_uint64(0), 3, pp, None, 10, None)
        assert st == L.UNSUPPORTED
        st, _ = _raw(fn, None, *head, 5, C.c_uint64(0), 3, None, None, 10, C.byref(nh))
        assert st == L.UNSUPPORTED
    # 4. no windows: OK with *n_hits = 0 (the input pointer is not looked at)
    for n, k in ((0, 0), (4, 5), (100, 0)):
        nh.value = 77
        st, _ = _raw(hits, None, None, n, k, C.c_uint64(0), 3, None, None, 0, C.byref(nh))
        assert st == L.OK and nh.value == 0
        nh.value = 77
        st, _ = _raw(packed, None, None, 8, n, k, C.c_uint64(0), 3, None, None, 0, C.byref(nh))
        assert st == L.OK and nh.value == 0
    # 5. a NULL input with windows; packed words not 8-byte aligned
    st, _ = _raw(hits, None, None, 256, 5, C.c_uint64(0), 3, pp, None, 10, C.byref(nh))
    assert st == L.UNSUPPORTED
    st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 8, 200, 5, C.c_uint64(0), 3, pp, None, 10, C.byref(nh))
    assert st == L.UNSUPPORTED
    # the _dev forms check their arguments before they need a device: a NULL context is refused first
    st, _ = _raw(lib.bitnuc_kmer_hdist_hits_dev, None, sp, 256, 5, C.c_uint64(0), 3, pp, None, 10, C.byref(nh))
    assert st == L.UNSUPPORTED
    st, _ = _raw(lib.bitnuc_kmer_hdist_hits_packed_dev, None, wp, 8, 256, 5, C.c_uint64(0), 3, pp, None, 10, C.byref(nh))
    assert st == L.UNSUPPORTED
