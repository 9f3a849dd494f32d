"""CPU tests of the mismatch histogram per query (bitnuc_kmer_hdist_hist / _hist_packed, bitnuc_kmer_pattern_hist / _hist_packed): the host path below
the cutoff through a NULL context against np.bincount over the oracle's scan (tests/hist_oracle.py) -- every k, every n_bins, query counts around the
query block; the argument checks in their documented order; all 256 byte values; patterns (singletons equal the exact form; N, R / Y and the empty set
against the pattern oracle); the three identities with count_multi, best and n - k + 1; and the host helpers (csrc/scan_hist_host.h) under ASan + UBSan
as a stand-alone program (tests/c/hist_host_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hist_oracle as ho
import pattern_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


def _junk(rng, queries, k):
    """junk above 2k"""
    if k == 32:
        return queries
    return queries | (rng.integers(0, 2**62, size=queries.size, dtype=np.uint64) << np.uint64(2 * k))


def _queries(rng, nq, k):
    return _junk(rng, rng.integers(0, 2**62, size=nq, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1), k)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "hist_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "hist host ok" in out.stdout


def test_host_path_every_k_and_every_n_bins_against_the_oracle(oracle):
    free = _free()
    rng = np.random.default_rng(0x4157)
    case = 0
    for k in range(1, 33):
        for nq in (1, 16, 17):
            for n in (0, k - 1, k, k + 1, 33, 1057):
                n_bins = 1 + case % 16  # every n_bins in 1 .. 16, many times over
                case += 1
                queries = _queries(rng, nq, k)
                s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
                want = ho.hist(oracle, s, k, queries, n_bins)
                if ho.roomy(n, k, n_bins):
                    ho.assert_rich(want, k, n_bins)
                got = free.kmer_hdist_hist(s, k, queries, n_bins)
                assert got.dtype == np.uint64 and got.shape == (nq, n_bins)
                assert np.array_equal(got, want), (k, nq, n, n_bins)
                words = po.pack_codes(po.codes_of_ascii(s), junk=0xDEADBEEFCAFEF00D)
                got = free.kmer_hdist_hist_packed(words if n else np.zeros(1, dtype=np.uint64), n, k, queries, n_bins)
                assert np.array_equal(got, want), (k, nq, n, n_bins)
    assert case >= 16 * 36


@pytest.mark.parametrize("n_bins", range(1, 17))
def test_every_n_bins_on_one_rich_reference(oracle, n_bins):
    free = _free()
    rng = np.random.default_rng(900 + n_bins)
    k, n, nq = 31, 8000, 5
    queries = _queries(rng, nq, k)
    s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
    want = ho.hist(oracle, s, k, queries, n_bins)
    ho.assert_rich(want, k, n_bins)
    assert np.array_equal(free.kmer_hdist_hist(s, k, queries, n_bins), want)
    assert np.array_equal(free.kmer_hdist_hist_packed(oracle.encode(s), n, k, queries, n_bins), want)


def test_n_bins_limits():
    from bitnuc_amd import _lib as L
    import bitnuc_amd as bn
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    words = np.zeros(8, dtype=np.uint64)
    q = np.zeros(2, dtype=np.uint64)
    p = np.zeros((2, 4), dtype=np.uint32)
    hist = np.full(40, 0xAB, dtype=np.uint64)
    sp, wp, qp, pp, hp = (C.c_void_p(a.ctypes.data) for a in (s, words, q, p, hist))
    for nb in (0, 17, 2**40):
        for fn, head, qq in ((lib.bitnuc_kmer_hdist_hist, (sp, 256, 5), qp), (lib.bitnuc_kmer_hdist_hist_packed, (wp, 8, 256, 5), qp),
                             (lib.bitnuc_kmer_pattern_hist, (sp, 256, 5), pp), (lib.bitnuc_kmer_pattern_hist_packed, (wp, 8, 256, 5), pp)):
            st, e = _raw(fn, None, *head, qq, 2, nb, hp)
            assert st == L.UNSUPPORTED and e.value == nb, (fn, nb)
    assert (hist == 0xAB).all()
    with pytest.raises(bn.NucleotideError) as ei:
        _free().kmer_hdist_hist(s, 5, [0, 1], 17)
    assert ei.value.kind == "Unsupported"
    with pytest.raises(bn.NucleotideError):
        _free().kmer_pattern_hist(s, 5, ["ACGTN"], 0)


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(8, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    hist = np.full(8 * 4 + 2, 0xAB, dtype=np.uint64)
    hp = C.c_void_p(hist.ctypes.data)
    for kind in ("exact", "pattern"):
        hist[:] = 0xAB
        if kind == "exact":
            host, packed = lib.bitnuc_kmer_hdist_hist, lib.bitnuc_kmer_hdist_hist_packed
            adev, pdev = lib.bitnuc_kmer_hdist_hist_async, lib.bitnuc_kmer_hdist_hist_packed_async
            q = np.zeros(8, dtype=np.uint64)
            misaligned = C.c_void_p(q.ctypes.data + 4)
        else:
            host, packed = lib.bitnuc_kmer_pattern_hist, lib.bitnuc_kmer_pattern_hist_packed
            adev, pdev = lib.bitnuc_kmer_pattern_hist_async, lib.bitnuc_kmer_pattern_hist_packed_async
            q = np.zeros((8, 4), dtype=np.uint32)
            q[:, 0] = 0xFFFFFFFF  # A at every position: the query AAAAA
            misaligned = C.c_void_p(q.ctypes.data + 2)
        qp = C.c_void_p(q.ctypes.data)
        # 1. the _async forms check the context first, whatever else is wrong
        st, e = _raw(adev, None, None, 256, 40, None, 70000, 99, None)
        assert st == L.UNSUPPORTED and e.value == 0
        st, e = _raw(pdev, None, None, 0, 100, 40, None, 70000, 99, None)
        assert st == L.UNSUPPORTED and e.value == 0
        # 2. k > 32, even with NULL pointers everywhere, too many bins and too many queries
        st, e = _raw(host, None, None, 256, 33, None, 70000, 99, None)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
        st, e = _raw(packed, None, None, 0, 100, 33, None, 70000, 99, None)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
        # 3. packed: too few words for n -> InvalidLength(n), before the bins and the queries
        st, e = _raw(packed, None, None, 3, 97, 5, None, 70000, 99, None)
        assert st == L.INVALID_LENGTH and e.value == 97
        # 4. the number of bins, before the number of queries: 0 and 17 with no queries, with too many
        for nq in (0, 70000):
            for nb in (0, 17):
                st, e = _raw(host, None, sp, 256, 5, None, nq, nb, None)
                assert st == L.UNSUPPORTED and e.value == nb
                st, e = _raw(packed, None, wp, 8, 256, 5, None, nq, nb, None)
                assert st == L.UNSUPPORTED and e.value == nb
        # 5. no queries: OK, nothing written, even with NULL arrays
        for fn, args in ((host, (sp, 256, 5)), (packed, (wp, 8, 256, 5))):
            st, e = _raw(fn, None, *args, None, 0, 4, None)
            assert st == L.OK
        # 6. too many queries -> Unsupported with the count, before the array checks
        st, e = _raw(host, None, sp, 256, 5, None, 65537, 4, None)
        assert st == L.UNSUPPORTED and e.value == 65537
        st, e = _raw(packed, None, wp, 8, 256, 5, None, 65537, 4, None)
        assert st == L.UNSUPPORTED and e.value == 65537
        # 7. hist / queries NULL or misaligned -> Unsupported, before the no-window case
        for qq, hh in ((None, hp), (qp, None), (misaligned, hp), (qp, C.c_void_p(hist.ctypes.data + 4))):
            st, e = _raw(host, None, sp, 3, 5, qq, 2, 4, hh)
            assert st == L.UNSUPPORTED and e.value == 0
            st, e = _raw(packed, None, wp, 8, 3, 5, qq, 2, 4, hh)
            assert st == L.UNSUPPORTED and e.value == 0
        assert (hist == 0xAB).all()
        # 8. no windows: zeros in [0, n_queries * n_bins) and nothing after them, before the reference is looked at
        for k, n in ((0, 100), (6, 5)):
            for fn, head in ((host, (None, n, k)), (packed, (None, 8, n, k))):
                hist[:] = 0xAB
                st, _ = _raw(fn, None, *head, qp, 8, 4, hp)
                assert st == L.OK and (hist[:32] == 0).all() and (hist[32:] == 0xAB).all()
        # 9. then a NULL reference, or packed words not 8-byte aligned
        hist[:] = 0xAB
        st, _ = _raw(host, None, None, 256, 5, qp, 8, 4, hp)
        assert st == L.UNSUPPORTED
        st, _ = _raw(packed, None, None, 8, 256, 5, qp, 8, 4, hp)
        assert st == L.UNSUPPORTED
        st, _ = _raw(packed, None, C.c_void_p(words.ctypes.data + 4), 7, 200, 5, qp, 8, 4, hp)
        assert st == L.UNSUPPORTED
        assert (hist == 0xAB).all()
        # and a valid call writes hist[0 .. n_queries * n_bins) only: AAAAA against ACGTACGT...: 63 windows each of ACGTA / CGTAC / GTACG / TACGT
        st, _ = _raw(host, None, sp, 256, 5, qp, 3, 4, hp)
        assert st == L.OK and (hist[12:] == 0xAB).all()
        assert hist[:12].reshape(3, 4).tolist() == [[0, 0, 0, 63]] * 3  # ACGTA is at 3; the others at 4 are counted nowhere


def test_all_256_byte_values_at_one_position():
    from bitnuc_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(256)
    k, n, at = 9, 300, 137
    base = ho.LUT[rng.integers(0, 4, size=n)].astype(np.uint8)
    q = _queries(rng, 3, k)
    valid = set(b"ACGTacgt")
    for b in range(256):
        s = base.copy()
        s[at] = b
        s[at + 50] = ord("?")  # a later invalid byte: the first one is reported
        hist = np.full(3 * 5 + 1, 0xAB, dtype=np.uint64)
        st, e = _raw(lib.bitnuc_kmer_hdist_hist, None, C.c_void_p(s.ctypes.data), n, k, C.c_void_p(q.ctypes.data), 3, 5, C.c_void_p(hist.ctypes.data))
        assert st == L.INVALID_BASE and (hist == 0xAB).all()  # outputs untouched on error
        assert (e.byte, e.index) == ((ord("?"), at + 50) if b in valid else (b, at)), b


def test_patterns_singletons_equal_the_exact_form_and_sets_follow_the_pattern_oracle(oracle):
    from bitnuc_amd import api
    free = _free()
    rng = np.random.default_rng(77)
    for k, n_bins in ((1, 1), (5, 6), (20, 8), (23, 9), (32, 16)):
        n, nq = 4000, 7
        queries = _queries(rng, nq, k)
        codes = ho.planted(rng, n, k, queries, n_bins)
        s = ho.ascii_of(rng, codes)
        exact = ho.hist(oracle, s, k, queries, n_bins)
        ho.assert_rich(exact, k, n_bins)
        singles = np.stack([api.pattern_from_2bit(int(q), k) for q in queries])
        assert np.array_equal(singles, np.stack([po.from_2bit(int(q), k) for q in queries]))
        assert np.array_equal(free.kmer_pattern_hist(s, k, singles, n_bins), exact)
        assert np.array_equal(free.kmer_pattern_hist_packed(po.pack_codes(codes), n, k, singles, n_bins), exact)
        # N, R / Y and the empty set at some positions of the queries' singletons
        pats = []
        for q in queries:
            sets = [{(int(q) >> (2 * i)) & 3} for i in range(k)]
            for i in range(k):
                r = int(rng.integers(0, 6))
                if r == 0:
                    sets[i] = {0, 1, 2, 3}
                elif r == 1:
                    sets[i] = {0, 2} if sets[i] <= {0, 2} else {1, 3}
                elif r == 2 and i % 7 == 3:
                    sets[i] = set()
            pats.append(po.from_sets(sets))
        pats = np.stack(pats)
        want = ho.pattern_hist(codes, pats, k, n_bins)
        assert want.sum() > 0
        assert np.array_equal(free.kmer_pattern_hist(s, k, pats, n_bins), want)
        assert np.array_equal(free.kmer_pattern_hist_packed(po.pack_codes(codes, junk=2**64 - 1), n, k, pats, n_bins), want)
    # IUPAC strings: a guide + NGG
    k, n_bins = 23, 5
    guides = ["ACGTTGCAAGGCTTAACGGTNGG", "TTGACCGTAAGGCATCGATANGG"]
    pats = np.stack([po.from_iupac(g) for g in guides])
    qs = np.array([ho.word([po.CODE[c] if c in po.CODE else 0 for c in g]) for g in guides], dtype=np.uint64)
    codes = ho.planted(rng, 6000, k, qs, n_bins)
    want = ho.pattern_hist(codes, pats, k, n_bins)
    ho.assert_rich(want, k, n_bins)
    assert np.array_equal(free.kmer_pattern_hist(ho.ascii_of(rng, codes), k, guides, n_bins), want)


def test_the_three_identities(oracle):
    import bitnuc_amd as bn
    free = _free()
    rng = np.random.default_rng(3)
    for k, n_bins in ((7, 8), (12, 13), (15, 16), (31, 16), (20, 4)):
        n, nq = 5000, 6
        queries = _queries(rng, nq, k)
        s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
        h = free.kmer_hdist_hist(s, k, queries, n_bins)
        assert np.array_equal(h, ho.hist(oracle, s, k, queries, n_bins))
        for t in range(n_bins):  # prefix sums are count_multi with taus = t
            assert np.array_equal(h[:, :t + 1].sum(axis=1), free.kmer_hdist_count_multi(s, k, queries, t)), (k, t)
        pos, dist = free.kmer_hdist_best(s, k, queries)  # the first non-zero bin is best's distance, when that is below n_bins
        for q in range(nq):
            nz = np.flatnonzero(h[q])
            if dist[q] < n_bins:
                assert nz.size and nz[0] == dist[q]
            else:
                assert nz.size == 0
        if n_bins > k:  # every distance has a bin: the bins sum to the number of windows
            assert (h.sum(axis=1) == n - k + 1).all()
    ps = bn.PackedSequence.__new__(bn.PackedSequence)  # (its constructor encodes on the device: the fields by hand)
    ps.data, ps.length, ps._ctx = oracle.encode(s), s.size, free
    assert np.array_equal(ps.kmer_hdist_hist(k, queries, n_bins), h)
    assert np.array_equal(ps.kmer_pattern_hist(k, np.stack([po.from_2bit(int(q), k) for q in queries]), n_bins), h)
    one = free.kmer_hdist_hist(s, k, int(queries[2]), n_bins)  # a scalar query: Q = 1
    assert one.shape == (1, n_bins) and np.array_equal(one[0], h[2])


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=100_000)].copy()
    k = 16
    for nq, host in ((10, True), (11, False)):  # 99,985 windows: x 10 < 2^20 <= x 11
        q = np.zeros(nq, dtype=np.uint64)
        hist = np.zeros(nq * 3, dtype=np.uint64)
        st, _ = _raw(lib.bitnuc_kmer_hdist_hist, None, C.c_void_p(s.ctypes.data), s.size, k, C.c_void_p(q.ctypes.data), nq, 3, C.c_void_p(hist.ctypes.data))
        assert st == (L.OK if host else L.UNSUPPORTED), nq
