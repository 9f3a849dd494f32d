"""CPU tests of the pattern queries (bitnuc_pattern_from_iupac / _from_2bit and the six host forms bitnuc_kmer_pattern_count_multi / _best / _hits
[_packed]) below the host cutoff, through ctypes with a NULL context: singleton patterns against the exact host forms, random sets (with empty sets and
N) against the brute force of tests/pattern_oracle.py, every IUPAC letter in both cases, the argument checks and their order, and the table builders,
an integer emulation of the contraction and the *_small twins under ASan + UBSan (tests/c/pattern_host_sanitize.cpp).  Exact integer equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pattern_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = np.frombuffer(b"ACGTacgt", dtype=np.uint8)


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


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_builders_emulation_and_small_forms_under_asan_ubsan(tmp_path):
    name = "pattern_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "pattern host ok" in out.stdout


def test_every_iupac_letter_in_both_cases():
    import bitnuc_amd as bn
    for ch, members in po.IUPAC.items():
        for letter in (ch, ch.lower()):
            for k, at in ((1, 0), (32, 31), (7, 3)):
                text = "N" * at + letter + "N" * (k - at - 1)
                got = bn.pattern_from_iupac(text)
                assert got.dtype == np.uint32 and got.shape == (4,)
                assert np.array_equal(got, po.from_iupac(text)), (letter, k, at)
                assert {c for c in range(4) if (int(got[c]) >> at) & 1} == {po.CODE[b] for b in members}
    assert np.array_equal(bn.pattern_from_iupac(b"acgtuRYswkmBDHVn"), po.from_iupac("ACGTURYSWKMBDHVN"))
    assert np.array_equal(bn.pattern_from_iupac(""), np.zeros(4, dtype=np.uint32))
    # every byte that is no IUPAC letter is refused with its index
    letters = set((("".join(po.IUPAC)) + "".join(po.IUPAC).lower()).encode())
    from bitnuc_amd import _lib as L
    out = np.zeros(4, dtype=np.uint32)
    for b in range(256):
        buf = np.frombuffer(b"NNN" + bytes([b]) + b"N", dtype=np.uint8).copy()
        out[:] = 0xAB
        st, e = _raw(L.load().bitnuc_pattern_from_iupac, _p(buf), 5, _p(out))
        if b in letters:
            assert st == L.OK, b
        else:
            assert st == L.INVALID_BASE and (e.byte, e.index) == (b, 3), b
            assert (out == 0xAB).all()


def test_from_2bit_is_the_pattern_of_singletons():
    import bitnuc_amd as bn
    rng = np.random.default_rng(5)
    for k in range(0, 33):
        q = int(rng.integers(0, 2**63, dtype=np.uint64)) * 2 + 1  # junk above 2k
        got = bn.pattern_from_2bit(q, k)
        assert np.array_equal(got, po.from_2bit(q, k)), k
        ones = (1 << k) - 1
        assert int(got[0]) | int(got[1]) | int(got[2]) | int(got[3]) == ones and sum(bin(int(x)).count("1") for x in got) == k


def _sequence(rng, n):
    codes = rng.integers(0, 4, size=n)
    return codes, LUT[codes + 4 * rng.integers(0, 2, size=n)].astype(np.uint8)


def _check_all_forms(free, codes, s, k, pats, taus, tag):
    """the six host forms on (s, its packed words) against the oracle"""
    n = len(codes)
    words = po.pack_codes(codes, junk=0xDEADBEEFCAFEF00D) if n else np.zeros(1, dtype=np.uint64)
    ds = [po.pdist(codes, p, k) for p in pats]
    want_counts = np.array([po.count(d, int(t)) for d, t in zip(ds, taus)], dtype=np.uint64)
    want_best = [po.best(d) for d in ds]
    wpos = np.array([b[0] for b in want_best], dtype=np.uint64)
    wdist = np.array([b[1] for b in want_best], dtype=np.uint8)
    P = np.ascontiguousarray(np.stack(pats))
    assert np.array_equal(free.kmer_pattern_count_multi(s, k, P, taus), want_counts), tag
    assert np.array_equal(free.kmer_pattern_count_multi_packed(words, n, k, P, taus), want_counts), tag
    for got in (free.kmer_pattern_best(s, k, P), free.kmer_pattern_best_packed(words, n, k, P)):
        assert np.array_equal(got[0], wpos) and np.array_equal(got[1], wdist), tag
    for p, d, t in list(zip(pats, ds, taus))[:3]:
        hp, hd, total = po.hits(d, int(t), 1 << 30)
        for got in (free.kmer_pattern_hits(s, k, p, int(t), with_dist=True), free.kmer_pattern_hits_packed(words, n, k, p, int(t), with_dist=True)):
            assert np.array_equal(got[0], hp) and np.array_equal(got[1], hd) and got[0].size == total, tag
    return want_counts, wpos, wdist


def test_singletons_equal_the_exact_host_forms_and_random_sets_equal_the_oracle():
    free = _free()
    rng = np.random.default_rng(0x9A77)
    for k in range(1, 33):
        for n in (0, k - 1, k, k + 1, 97):
            codes, s = _sequence(rng, n)
            words = po.pack_codes(codes) if n else np.zeros(1, dtype=np.uint64)
            # singletons: a window of the sequence, a random query, both with junk above 2k
            queries = rng.integers(0, 2**63, size=3, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            if n >= k:
                at = int(rng.integers(0, n - k + 1))
                w = sum(int(c) << (2 * b) for b, c in enumerate(codes[at:at + k]))
                queries[0] = np.uint64(w if k == 32 else w | ((int(queries[0]) << (2 * k)) & (2**64 - 1)))
            taus = np.array([0, k // 2, k], dtype=np.uint32)
            singles = [po.from_2bit(int(q), k) for q in queries]
            counts, pos, dist = _check_all_forms(free, codes, s, k, singles, taus, ("single", k, n))
            assert np.array_equal(counts, free.kmer_hdist_count_multi(s, k, queries, taus))
            assert np.array_equal(counts, free.kmer_hdist_count_multi_packed(words, n, k, queries, taus))
            epos, edist = free.kmer_hdist_best(s, k, queries)
            assert np.array_equal(pos, epos) and np.array_equal(dist, edist)
            for q, p, t in zip(queries, singles, taus):
                a = free.kmer_hdist_hits(s, k, int(q), int(t), with_dist=True)
                b = free.kmer_pattern_hits(s, k, p, int(t), with_dist=True)
                c = free.kmer_hdist_hits_packed(words, n, k, int(q), int(t), with_dist=True)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0])
            # random sets with empty sets and N; all-N; all-empty; one {T}, one {A, T}
            pats = [po.from_sets(po.random_sets(rng, k)) for _ in range(3)]
            pats += [po.from_iupac("N" * k), po.from_sets([set()] * k), po.from_sets([{3}] * k), po.from_sets([{0, 3}] * k)]
            taus = np.array([0, 1, k - 1, 0, k - 1, k // 3, 2**32 - 1], dtype=np.uint32)
            _check_all_forms(free, codes, s, k, pats, taus, ("sets", k, n))


def test_pam_shapes_iupac_strings_and_the_sequence_method():
    import bitnuc_amd as bn
    free = _free()
    rng = np.random.default_rng(77)
    n, k = 4000, 23
    codes, s = _sequence(rng, n)
    guide = "".join("ACGT"[c] for c in rng.integers(0, 4, size=20))
    site = [po.CODE[ch] for ch in guide] + [1, 2, 2]  # guide + CGG
    for at in (0, 777, n - k):
        codes[at:at + k] = site
    codes[777 + 3] ^= 1  # one mismatch in the guide part
    codes[n - k + 21] = 0  # the last site's PAM is broken: GG -> AG
    s = LUT[codes].copy()
    pats = [guide + "NGG", guide + "NRG", "N" * 20 + "NGG"]
    taus = [1, 1, 0]
    counts = free.kmer_pattern_count_multi(s, k, pats, taus)
    P = [po.from_iupac(p) for p in pats]
    want = [po.count(po.pdist(codes, p, k), t) for p, t in zip(P, taus)]
    assert list(counts) == want and want[0] >= 2 and want[1] >= 3
    pos = free.kmer_pattern_hits(s, k, pats[0], 1)
    assert 0 in pos and 777 in pos and (n - k) in pos  # one guide mismatch, one PAM mismatch: both within tau = 1
    exact = free.kmer_pattern_hits(s, k, pats[0], 0)
    assert 0 in exact and 777 not in exact and (n - k) not in exact
    relaxed = free.kmer_pattern_hits(s, k, pats[1], 0)  # R accepts the A
    assert 0 in relaxed and 777 not in relaxed and (n - k) in relaxed
    bpos, bdist = free.kmer_pattern_best(s, k, pats[:2])
    assert list(bpos) == [0, 0] and list(bdist) == [0, 0]
    ps = bn.PackedSequence.__new__(bn.PackedSequence)  # (its constructor encodes on the device: the fields by hand)
    ps.data, ps.length, ps._ctx = po.pack_codes(codes), n, free
    assert np.array_equal(ps.kmer_pattern_count_multi(k, pats, taus), counts)
    assert np.array_equal(ps.kmer_pattern_hits(k, pats[0], 1), pos)
    assert np.array_equal(ps.kmer_pattern_best(k, pats[:2])[0], bpos)
    with pytest.raises(ValueError):
        free.kmer_pattern_count_multi(s, k, ["ACGT"], 0)  # four letters for k = 23


def test_invalid_reference_byte_first_index_outputs_untouched():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGTACGTAC" * 50, dtype=np.uint8).copy()
    s[123] = ord("N")  # N is a pattern letter, not a reference base
    s[400] = ord("x")
    P = np.ascontiguousarray(np.stack([po.from_iupac("NNNNNNN")] * 3))
    taus = np.zeros(3, dtype=np.uint32)
    out = np.full(4, 0xAB, dtype=np.uint64)
    st, e = _raw(lib.bitnuc_kmer_pattern_count_multi, None, _p(s), s.size, 7, _p(P), _p(taus), 3, _p(out))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 123) and (out == 0xAB).all()
    dist = np.full(4, 0xAB, dtype=np.uint8)
    st, e = _raw(lib.bitnuc_kmer_pattern_best, None, _p(s), s.size, 7, _p(P), 3, _p(out), _p(dist))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 123) and (out == 0xAB).all() and (dist == 0xAB).all()
    nh = C.c_uint64(0xAB)
    st, e = _raw(lib.bitnuc_kmer_pattern_hits, None, _p(s), s.size, 7, _p(P), 7, _p(out), _p(dist), 4, C.byref(nh))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), 123) and (out == 0xAB).all() and nh.value == 0xAB


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    words = np.zeros(8, dtype=np.uint64)
    raw = np.zeros(4 * 8 + 1, dtype=np.uint32)
    P = raw[:32]
    P[:] = np.tile(po.from_iupac("NNNNN"), 8)
    taus = np.zeros(8, dtype=np.uint32)
    out = np.full(10, 0xAB, dtype=np.uint64)
    dist = np.full(16, 0xAB, dtype=np.uint8)
    pat = np.zeros(4, dtype=np.uint32)
    # the converters: k = 33 before any letter is read (a NULL pointer, an invalid letter), then the letters
    st, e = _raw(lib.bitnuc_pattern_from_iupac, None, 33, _p(pat))
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    bad = np.frombuffer(b"?" * 33, dtype=np.uint8).copy()
    st, e = _raw(lib.bitnuc_pattern_from_iupac, _p(bad), 33, _p(pat))
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    st, e = _raw(lib.bitnuc_pattern_from_iupac, _p(bad), 32, _p(pat))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("?"), 0)
    letters = np.frombuffer(b"ACGTNX", dtype=np.uint8).copy()
    st, e = _raw(lib.bitnuc_pattern_from_iupac, _p(letters), 6, _p(pat))
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("X"), 5)
    st, e = _raw(lib.bitnuc_pattern_from_2bit, C.c_uint64(0), 33, _p(pat))
    assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    assert _raw(lib.bitnuc_pattern_from_2bit, C.c_uint64(0), 5, None)[0] == L.UNSUPPORTED
    assert _raw(lib.bitnuc_pattern_from_iupac, _p(letters), 5, None)[0] == L.UNSUPPORTED

    cm, cmp_ = lib.bitnuc_kmer_pattern_count_multi, lib.bitnuc_kmer_pattern_count_multi_packed
    be, bep = lib.bitnuc_kmer_pattern_best, lib.bitnuc_kmer_pattern_best_packed
    hi, hip_ = lib.bitnuc_kmer_pattern_hits, lib.bitnuc_kmer_pattern_hits_packed
    nh = C.c_uint64(0xAB)
    # 1. the _async forms check the context first, whatever else is wrong
    for fn, args in ((lib.bitnuc_kmer_pattern_count_multi_async, (None, 256, 40, None, None, 70000, None)),
                     (lib.bitnuc_kmer_pattern_count_multi_packed_async, (None, 0, 100, 40, None, None, 70000, None)),
                     (lib.bitnuc_kmer_pattern_best_async, (None, 256, 40, None, 70000, None, None)),
                     (lib.bitnuc_kmer_pattern_best_packed_async, (None, 0, 100, 40, None, 70000, None, None)),
                     (lib.bitnuc_kmer_pattern_hits_async, (None, 256, 40, None, 0, None, None, 5, None)),
                     (lib.bitnuc_kmer_pattern_hits_packed_async, (None, 0, 100, 40, None, 0, None, None, 5, None))):
        st, e = _raw(fn, None, *args)
        assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with NULL pointers everywhere and too many queries
    for fn, args in ((cm, (None, 256, 33, None, None, 70000, None)), (cmp_, (None, 0, 100, 33, None, None, 70000, None)),
                     (be, (None, 256, 33, None, 70000, None, None)), (bep, (None, 0, 100, 33, None, 70000, None, None)),
                     (hi, (None, 256, 33, None, 0, None, None, 5, None)), (hip_, (None, 0, 100, 33, None, 0, None, None, 5, None))):
        st, e = _raw(fn, None, *args)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # 3. packed: too few words for n -> InvalidLength(n), before the query checks
    for fn, args in ((cmp_, (None, 3, 97, 5, None, None, 70000, None)), (bep, (None, 3, 97, 5, None, 70000, None, None)),
                     (hip_, (None, 3, 97, 5, None, 0, None, None, 5, None))):
        st, e = _raw(fn, None, *args)
        assert st == L.INVALID_LENGTH and e.value == 97
    # 4. n_queries == 0: OK, nothing written, even with NULL arrays
    assert _raw(cm, None, _p(s), 256, 5, None, None, 0, None)[0] == L.OK
    assert _raw(cmp_, None, _p(words), 8, 256, 5, None, None, 0, None)[0] == L.OK
    assert _raw(be, None, _p(s), 256, 5, None, 0, None, None)[0] == L.OK
    assert _raw(bep, None, _p(words), 8, 256, 5, None, 0, None, None)[0] == L.OK
    # 5. n_queries > BITNUC_MAX_QUERIES -> Unsupported with the count, before the array checks
    for fn, args in ((cm, (_p(s), 256, 5, None, None, 65537, None)), (cmp_, (_p(words), 8, 256, 5, None, None, 65537, None)),
                     (be, (_p(s), 256, 5, None, 65537, None, None)), (bep, (_p(words), 8, 256, 5, None, 65537, None, None))):
        st, e = _raw(fn, None, *args)
        assert st == L.UNSUPPORTED and e.value == 65537
    # 6. NULL or misaligned arrays (patterns: 4-byte aligned is enough, 2 is not), before the no-window case
    p2 = C.c_void_p(P.ctypes.data + 2)
    for pp, tp, op in ((None, _p(taus), _p(out)), (_p(P), None, _p(out)), (_p(P), _p(taus), None), (p2, _p(taus), _p(out)),
                       (_p(P), C.c_void_p(taus.ctypes.data + 2), _p(out)), (_p(P), _p(taus), C.c_void_p(out.ctypes.data + 4))):
        assert _raw(cm, None, _p(s), 3, 5, pp, tp, 2, op)[0] == L.UNSUPPORTED
        assert _raw(cmp_, None, _p(words), 8, 3, 5, pp, tp, 2, op)[0] == L.UNSUPPORTED
    for pp, op, dp in ((None, _p(out), _p(dist)), (_p(P), None, _p(dist)), (_p(P), _p(out), None), (p2, _p(out), _p(dist)),
                       (_p(P), C.c_void_p(out.ctypes.data + 4), _p(dist))):
        assert _raw(be, None, _p(s), 3, 5, pp, 2, op, dp)[0] == L.UNSUPPORTED
        assert _raw(bep, None, _p(words), 8, 3, 5, pp, 2, op, dp)[0] == L.UNSUPPORTED
    # hits: n_hits NULL, pos NULL with cap > 0, a NULL pattern -- before the no-window case
    for pp, op, cap, nhp in ((_p(P), _p(out), 5, None), (_p(P), None, 5, C.byref(nh)), (None, _p(out), 5, C.byref(nh)), (None, None, 0, C.byref(nh))):
        assert _raw(hi, None, _p(s), 3, 5, pp, 0, op, None, cap, nhp)[0] == L.UNSUPPORTED
        assert _raw(hip_, None, _p(words), 8, 3, 5, pp, 0, op, None, cap, nhp)[0] == L.UNSUPPORTED
    assert nh.value == 0xAB
    # patterns at 4 mod 8 are fine
    P4 = raw[1:33]
    P4[:] = np.tile(po.from_iupac("NNNNN"), 8)
    assert P4.ctypes.data - P.ctypes.data == 4
    out[:] = 0xAB
    assert _raw(cm, None, _p(s), 256, 5, _p(P4), _p(taus), 3, _p(out))[0] == L.OK
    assert list(out[:3]) == [252] * 3 and (out[3:] == 0xAB).all()  # all-N: every window counts, nothing past n_queries
    # 7. no windows: zero counts, the best match's fill, *n_hits = 0 -- before the reference is looked at
    for k, n in ((0, 100), (6, 5)):
        out[:] = 0xAB
        assert _raw(cm, None, None, n, k, _p(P), _p(taus), 8, _p(out))[0] == L.OK and (out[:8] == 0).all() and (out[8:] == 0xAB).all()
        out[:] = 0xAB
        dist[:] = 0xAB
        assert _raw(be, None, None, n, k, _p(P), 8, _p(out), C.c_void_p(dist.ctypes.data + 1))[0] == L.OK
        assert (out[:8] == po.NO_POS).all() and (out[8:] == 0xAB).all() and dist[0] == 0xAB and (dist[1:9] == 0xFF).all() and (dist[9:] == 0xAB).all()
        nh.value = 0xAB
        assert _raw(hi, None, None, n, k, _p(P), 0, _p(out), None, 5, C.byref(nh))[0] == L.OK and nh.value == 0
        nh.value = 0xAB
        assert _raw(hip_, None, None, 8, n, k, _p(P), 0, _p(out), None, 5, C.byref(nh))[0] == L.OK and nh.value == 0
    # 8. then a NULL reference, or packed words not 8-byte aligned
    assert _raw(cm, None, None, 256, 5, _p(P), _p(taus), 8, _p(out))[0] == L.UNSUPPORTED
    assert _raw(be, None, None, 256, 5, _p(P), 8, _p(out), _p(dist))[0] == L.UNSUPPORTED
    assert _raw(hi, None, None, 256, 5, _p(P), 0, _p(out), None, 5, C.byref(nh))[0] == L.UNSUPPORTED
    w4 = C.c_void_p(words.ctypes.data + 4)
    assert _raw(cmp_, None, w4, 7, 200, 5, _p(P), _p(taus), 8, _p(out))[0] == L.UNSUPPORTED
    assert _raw(bep, None, w4, 7, 200, 5, _p(P), 8, _p(out), _p(dist))[0] == L.UNSUPPORTED
    assert _raw(hip_, None, w4, 7, 200, 5, _p(P), 0, _p(out), None, 5, C.byref(nh))[0] == L.UNSUPPORTED
    # cap = 0 counts without writing; cap < n_hits writes the first cap and nothing after them
    acgt = po.from_iupac("ACGTA")
    for fn, head in ((hi, (_p(s), 256, 5)), (hip_, (_p(po.pack_codes([0, 1, 2, 3] * 64)), 8, 256, 5))):
        out[:] = 0xAB
        dist[:] = 0xAB
        nh.value = 0xAB
        assert _raw(fn, None, *head, _p(acgt), 0, None, None, 0, C.byref(nh))[0] == L.OK and nh.value == 63
        assert _raw(fn, None, *head, _p(acgt), 0, _p(out), _p(dist), 4, C.byref(nh))[0] == L.OK and nh.value == 63
        assert list(out[:4]) == [0, 4, 8, 12] and (out[4:] == 0xAB).all() and (dist[:4] == 0).all() and (dist[4:] == 0xAB).all()


def test_host_cutoff_is_judged_on_windows_times_queries():
    """Below the cutoff (1 Mi windows x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=100_000)].copy()
    k = 16
    for nq, host in ((10, True), (11, False)):  # 99,985 windows: x 10 < 2^20 <= x 11
        P = np.zeros((nq, 4), dtype=np.uint32)
        taus = np.zeros(nq, dtype=np.uint32)
        out = np.zeros(nq, dtype=np.uint64)
        st, _ = _raw(lib.bitnuc_kmer_pattern_count_multi, None, _p(s), s.size, k, _p(P), _p(taus), nq, _p(out))
        assert st == (L.OK if host else L.UNSUPPORTED), nq
        assert not host or (out == 0).all()  # the empty pattern at tau 0 matches nothing
