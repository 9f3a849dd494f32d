"""CPU tests of the sliding k-mer Hamming scan and its fused count on PACKED words (bitnuc_kmer_hdist_scan_packed / _count_packed):
the host path below the cutoff against the oracle's ASCII scan of the decoded sequence, the argument checks and their order, and an
integer emulation of the matrix-core contraction the kernels run (tests/c/packed_scan_emulate.cpp) under ASan + UBSan."""
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


def _junk_words(rng, n):
    """ceil(n/32) random words: every bit random, including the bits above 2n in the last word"""
    return rng.integers(0, 2**64, size=(n + 31) // 32, dtype=np.uint64, endpoint=False)


def _taus(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 2**32 - 1})


def _oracle_dist(oracle, words, n, k, query):
    return oracle.kmer_hdist_scan(oracle.decode(words, n), k, query)


def test_packed_contraction_emulated_under_asan_ubsan(tmp_path):
    """Table, row scales and start values applied to operands built in the packed K order: the distance byte fields, the threshold bits and
    the hit count are exact for every k in 1..32 and tau in {0, 1, k-1, k, k+1, 2^32-1}, with every partial sum below 2^24."""
    exe = str(tmp_path / "packed_scan_emulate")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", "packed_scan_emulate.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "packed scan emulation ok" in out.stdout


def test_host_path_every_k_and_small_n_against_the_oracle(oracle):
    free = _free()
    rng = np.random.default_rng(0xB17C0DE)
    for k in range(1, 33):
        query = int(rng.integers(0, 2**64, dtype=np.uint64))  # junk above 2k
        for n in range(0, 201):
            words = _junk_words(rng, n)
            want = _oracle_dist(oracle, words, n, k, query)
            got = free.kmer_hdist_scan_packed(words, n, k, query)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (k, n)
            if n % 25 == 0 or n in (k - 1, k, k + 1):
                for tau in _taus(k):
                    assert free.kmer_hdist_count_packed(words, n, k, query, tau) == int((want <= tau).sum()), (k, n, tau)


@pytest.mark.parametrize("n", [1055, 1056, 1057, 3001, 4096 + 31, 4096 + 33, 6000])
def test_host_path_a_few_thousand_bases(oracle, n):
    free = _free()
    rng = np.random.default_rng(n)
    for k in (1, 7, 16, 31, 32):
        words = _junk_words(rng, n)
        # most windows hit: the query's bases repeated, a tenth of them changed
        if k == 31:
            q = rng.integers(0, 4, size=k)
            bases = np.resize(q, n).astype(np.uint64)
            flip = rng.random(n) < 0.1
            bases[flip] = rng.integers(0, 4, size=int(flip.sum()))
            words = np.zeros((n + 31) // 32, dtype=np.uint64)
            for i, b in enumerate(bases):
                words[i // 32] |= np.uint64(int(b) << (2 * (i % 32)))
            query = int(sum(int(b) << (2 * i) for i, b in enumerate(q))) | (3 << 62)  # junk above 2k
        else:
            query = int(rng.integers(0, 2**64, dtype=np.uint64))
        want = _oracle_dist(oracle, words, n, k, query)
        assert np.array_equal(free.kmer_hdist_scan_packed(words, n, k, query), want), (n, k)
        for tau in _taus(k):
            assert free.kmer_hdist_count_packed(words, n, k, query, tau) == int((want <= tau).sum()), (n, k, tau)


def test_packed_sequence_scans_its_own_words(oracle):
    from bitnuc_amd import PackedSequence
    rng = np.random.default_rng(7)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=777))
    ps = PackedSequence(seq, ctx=_free())
    query = int(rng.integers(0, 2**62))
    want = oracle.kmer_hdist_scan(seq, 21, query)
    assert np.array_equal(ps.kmer_hdist_scan(21, query), want)
    assert ps.kmer_hdist_count(21, query, 9) == int((want <= 9).sum())


def test_module_level_function_is_exported():
    import bitnuc_amd
    assert "kmer_hdist_scan_packed" in bitnuc_amd.__all__ and callable(bitnuc_amd.kmer_hdist_scan_packed)


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    words = np.zeros(8, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    dist = np.zeros(512, dtype=np.uint8)
    dp = C.c_void_p(dist.ctypes.data)
    cnt = C.c_uint64(77)
    scan, count = lib.bitnuc_kmer_hdist_scan_packed, lib.bitnuc_kmer_hdist_count_packed
    # 1. k > 32 comes first, even with too few words and NULL pointers
    for fn, tail in ((scan, (None,)), (count, (3, None))):
        st, e = _raw(fn, None, None, 0, 100, 33, C.c_uint64(0), *tail)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 2. too few words for n: InvalidLength(n), before the no-window case and the pointer checks
    for k in (0, 5):
        st, e = _raw(scan, None, None, 3, 97, k, C.c_uint64(0), None)
        assert st == L.INVALID_LENGTH and e.value == 97
        st, e = _raw(count, None, None, 3, 97, k, C.c_uint64(0), 3, None)
        assert st == L.INVALID_LENGTH and e.value == 97
    # 3. no windows: OK (NULL words / dist are not looked at); the count writes 0
    for n, k in ((0, 0), (0, 5), (4, 5), (100, 0)):
        st, _ = _raw(scan, None, None, 8, n, k, C.c_uint64(0), None)
        assert st == L.OK
        cnt.value = 77
        st, _ = _raw(count, None, wp, 8, n, k, C.c_uint64(0), 3, C.byref(cnt))
        assert st == L.OK and cnt.value == 0
    # 4. NULL or misaligned pointers: Unsupported
    st, _ = _raw(scan, None, None, 8, 100, 5, C.c_uint64(0), dp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(scan, None, wp, 8, 100, 5, C.c_uint64(0), None)
    assert st == L.UNSUPPORTED
    st, _ = _raw(scan, None, C.c_void_p(words.ctypes.data + 4), 7, 100, 5, C.c_uint64(0), dp)
    assert st == L.UNSUPPORTED
    st, _ = _raw(count, None, wp, 8, 100, 5, C.c_uint64(0), 3, None)
    assert st == L.UNSUPPORTED
    st, _ = _raw(count, None, C.c_void_p(words.ctypes.data + 4), 7, 100, 5, C.c_uint64(0), 3, C.byref(cnt))
    assert st == L.UNSUPPORTED
    # a words pointer at 8 mod 16 is fine, and dist may sit at any byte offset
    st, _ = _raw(scan, None, C.c_void_p(words.ctypes.data + 8), 7, 100, 5, C.c_uint64(0), C.c_void_p(dist.ctypes.data + 3))
    assert st == L.OK
    # above the host cutoff without a context: fails as bitnuc_hdist does
    big = np.zeros((1 << 20) // 32, dtype=np.uint64)
    st, _ = _raw(scan, None, C.c_void_p(big.ctypes.data), big.size, 1 << 20, 31, C.c_uint64(0), C.c_void_p(np.zeros(1 << 20, np.uint8).ctypes.data))
    assert st == L.UNSUPPORTED
    st, _ = _raw(count, None, C.c_void_p(big.ctypes.data), big.size, 1 << 20, 31, C.c_uint64(0), 3, C.byref(cnt))
    assert st == L.UNSUPPORTED


def test_python_errors_are_the_reference_vocabulary():
    from bitnuc_amd import NucleotideError
    free = _free()
    with pytest.raises(NucleotideError) as e:
        free.kmer_hdist_scan_packed(np.zeros(1, np.uint64), 32, 33, 0)
    assert e.value.kind == "SequenceTooLong" and e.value.len == 33
    with pytest.raises(NucleotideError) as e:
        free.kmer_hdist_count_packed(np.zeros(1, np.uint64), 33, 4, 0, 1)
    assert e.value.kind == "InvalidLength" and e.value.len == 33
    assert free.kmer_hdist_scan_packed(np.zeros(0, np.uint64), 0, 4, 0).size == 0
    assert free.kmer_hdist_count_packed(np.zeros(1, np.uint64), 3, 4, 0, 1) == 0
