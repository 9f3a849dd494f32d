"""CPU tests of the indel-tolerant hit list (bitnuc_kmer_edist_hits, its _packed form and the pattern twins): the host path below the cutoff, through a
NULL context, against kmer_edist_oracle.ends() (the plain DP; the host path is the bit-parallel recurrence): pos = nonzero(e <= tau) + 1,
dist = e[pos - 1] -- every k in 1 .. 32 at n in {k, k + 1, 2k, 63, 64, 65, 200}; tau in {0, 1, k - 1, k, 2^32 - 1}; cap in {0, 1, total - 1, total,
total + 1} with guard words behind cap; hit_dist NULL; a hand-checked insertion and a hand-checked deletion; a hit at j = 1 and at j = n; a pattern with
N positions and an empty set; singleton patterns equal to the exact form; *n_hits equal to bitnuc_kmer_edist_count_multi with one query at every point;
the no-windows fill; an invalid byte with the outputs untouched; the argument checks in their documented order for both query kinds; the cutoff, judged
on n; the host helpers under ASan + UBSan in a stand-alone program (tests/c/kmer_edist_hits_host_sanitize.cpp).  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_edist_hits_oracle as ho
import kmer_edist_oracle as ko
import pattern_oracle as po
import reads_best_oracle as ro
import reads_edist_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _ascii(codes, rng=None):
    s = ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)
    if rng is not None:
        s[rng.random(s.size) < 0.3] |= 0x20  # about 30 % lowercase
    return s


class Out:
    """end (u64, cap entries) inside GUARD guard words, hit_dist (u8, cap entries) at byte offset 1 of its buffer, n_hits"""

    def __init__(self, cap):
        self.cap = cap
        self.w = np.full(cap + 2 * GUARD, FILL64, dtype=np.uint64)
        self.d = np.full(1 + cap + GUARD, 0x5A, dtype=np.uint8)
        self.n = np.full(3, FILL64, dtype=np.uint64)

    def wp(self):
        return C.c_void_p(self.w.ctypes.data + 8 * GUARD)

    def dp(self):
        return C.c_void_p(self.d.ctypes.data + 1)

    def np_(self):
        return C.c_void_p(self.n.ctypes.data + 8)

    def untouched(self):
        return bool((self.w == FILL64).all() and (self.d == 0x5A).all() and (self.n == FILL64).all())

    def read(self):
        """(total, end[0 .. min(cap, total)), dist likewise); everything else must be untouched"""
        assert self.n[0] == FILL64 and self.n[2] == FILL64
        total = int(self.n[1])
        m = min(self.cap, total)
        assert (self.w[:GUARD] == FILL64).all() and (self.w[GUARD + m:] == FILL64).all(), "end written outside [0, min(cap, total))"
        assert (self.d[:1] == 0x5A).all() and (self.d[1 + m:] == 0x5A).all(), "hit_dist written outside [0, min(cap, total))"
        return total, self.w[GUARD:GUARD + m].copy(), self.d[1:1 + m].copy()


def _fn(form, pattern):
    from bitnuc_amd import _lib as L
    return getattr(L.load(), "bitnuc_kmer_" + ("pattern_" if pattern else "") + "edist_hits" + ("" if form == "ascii" else "_packed"))


def _hits(form, src, n, k, query, tau, cap, pattern=False, with_dist=True, ctx=None):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    head = (C.c_void_p(src.ctypes.data), src.size, n) if form == "packed" else (C.c_void_p(src.ctypes.data), n)
    if pattern:
        p = np.ascontiguousarray(np.asarray(query, dtype=np.uint32).reshape(4))
        q = C.c_void_p(p.ctypes.data)
    else:
        q = C.c_uint64(int(query))
    o = Out(cap)
    err = L.BitnucErr()
    st = _fn(form, pattern)(ctx, *head, k, q, int(tau), o.wp() if cap else None, o.dp() if (with_dist and cap) else None, cap,
                            C.cast(o.np_(), C.POINTER(C.c_uint64)), C.byref(err))
    return st, err, o


def _count1(form, src, n, k, query, tau, pattern=False):
    free = _free()
    name = "kmer_" + ("pattern_" if pattern else "") + "edist_count_multi" + ("" if form == "ascii" else "_packed")
    args = (src, k) if form == "ascii" else (src, n, k)
    return int(getattr(free, name)(*args, [query], [tau])[0])


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "kmer_edist_hits_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "kmer edist hits host ok" in out.stdout


@pytest.mark.parametrize("k0", [1, 9, 17, 25])
def test_host_path_against_the_dp(k0):
    """k = k0 .. k0 + 7 (1 .. 32 over the four cases) at n in {k, k + 1, 2k, 63, 64, 65, 200}, tau in {0, 1, k - 1, k, 2^32 - 1}, cap in {0, 1, total - 1,
    total, total + 1} (rotating; every cap at every k), both layouts, both query kinds; *n_hits against the count with one query at every point"""
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0xE1D7 + k0)
    turn = 0
    for k in range(k0, k0 + 8):
        for n in sorted({k, k + 1, 2 * k, 63, 64, 65, 200}):
            if n < k:
                continue
            query = int(ro.random_queries(rng, 1, k)[0])
            codes = rng.integers(0, 4, size=n)
            c = eo.plant(rng, ro.query_codes(query, k), int(rng.integers(0, 3)))[:n]
            at = int(rng.integers(0, n - len(c) + 1))
            codes[at:at + len(c)] = c
            s, words = _ascii(codes, rng), po.pack_codes(codes, junk=0xDEADBEEFDEADBEEF)  # junk above 2n
            sing = po.from_2bit(query, k)
            e = ko.ends(codes, k, sing)
            for tau in sorted({0, 1, max(k - 1, 0), k, 2**32 - 1}):
                pos, dist = ho.of_ends(e, tau)
                total = pos.size
                assert tau < k or total == n  # tau >= k: every end
                caps = sorted({0, 1, max(total - 1, 0), total, total + 1})
                for form, src in (("ascii", s), ("packed", words)):
                    assert _count1(form, src, n, k, query, tau) == total
                    for pattern, q in ((False, query | ((1 << 63) if k < 31 else 0)), (True, sing)):  # junk above 2k
                        for cap in (caps if (turn % 5 == 0) else [caps[turn % len(caps)]]):
                            turn += 1
                            st, _, o = _hits(form, src, n, k, q, tau, cap, pattern)
                            got = o.read()
                            m = min(cap, total)
                            assert st == L.OK and got[0] == total and np.array_equal(got[1], pos[:m]) and np.array_equal(got[2], dist[:m]), (form, pattern, k, n, tau, cap)
                        turn += 1


def test_every_cap_with_guards_and_without_hit_dist():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0xCA9)
    k, n = 12, 200
    query = int(ro.random_queries(rng, 1, k)[0])
    codes = rng.integers(0, 4, size=n)
    for at, d in ((20, 0), (90, 1), (150, 2)):
        c = eo.plant(rng, ro.query_codes(query, k), d)
        codes[at:at + len(c)] = c
    s, words = _ascii(codes, rng), po.pack_codes(codes, junk=2**64 - 1)
    sing = po.from_2bit(query, k)
    for tau in (0, 2, k - 1):
        pos, dist = ho.hits(codes, k, sing, tau)
        total = pos.size
        assert total >= 1
        for cap in sorted({0, 1, total - 1, total, total + 1}):
            m = min(cap, total)
            for form, src in (("ascii", s), ("packed", words)):
                for pattern, q in ((False, query), (True, sing)):
                    for with_dist in (True, False):
                        st, _, o = _hits(form, src, n, k, q, tau, cap, pattern, with_dist)
                        got = o.read()
                        assert st == L.OK and got[0] == total and np.array_equal(got[1], pos[:m])
                        assert np.array_equal(got[2], dist[:m]) if with_dist else (o.d == 0x5A).all()


def test_an_insertion_and_a_deletion_by_hand():
    """query ACGTACGTAC (k = 10) in a reference of G only.
    Insertion: ACGTA + T + CGTAC from 0-based base 5 ends at 5 + 11 = 16 with distance 1; its neighbours at 15 and 17 have distance 2.
    Deletion: ACGT + CGTAC (the A dropped) from 0-based base 30 ends at 30 + 9 = 39 with distance 1."""
    free = _free()
    k = 10
    q = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1])
    n = 60
    codes = np.full(n, 2)
    ins = np.concatenate([q[:5], [3], q[5:]])
    codes[5:5 + 11] = ins
    dele = np.concatenate([q[:4], q[5:]])
    codes[30:30 + 9] = dele
    query = ro.word_of(q)
    s = _ascii(codes)
    pos, dist = free.kmer_edist_hits(s, k, query, 1, with_dist=True)
    assert list(pos) == [16, 39] and list(dist) == [1, 1]
    assert pos.dtype == np.uint64 and dist.dtype == np.uint8
    pos2, dist2 = free.kmer_edist_hits(s, k, query, 2, with_dist=True)
    want = ho.hits(codes, k, po.from_2bit(query, k), 2)
    assert np.array_equal(pos2, want[0]) and np.array_equal(dist2, want[1])
    assert {15, 16, 17}.issubset(set(int(x) for x in pos2)) and {38, 39, 40}.issubset(set(int(x) for x in pos2))  # neighbours of a good end are hits too
    assert dict(zip(pos2.tolist(), dist2.tolist()))[15] == 2 and dict(zip(pos2.tolist(), dist2.tolist()))[17] == 2
    assert list(free.kmer_edist_hits(s, k, query, 0)) == []  # no exact copy
    assert np.array_equal(free.kmer_edist_hits_packed(po.pack_codes(codes), n, k, query, 1), [16, 39])


def test_a_hit_at_the_first_and_at_the_last_end():
    free = _free()
    k, n = 8, 50
    q = np.array([0, 1, 2, 3, 3, 2, 1, 0])
    codes = np.full(n, 1)  # C: E(1) = k - 1 only where the query's last base matches; the last base is A here
    codes[0] = 0  # base 1 = A matches the last position: E(1) = k - 1
    codes[n - k:] = q  # an exact copy ends at j = n
    query = ro.word_of(q)
    sing = po.from_2bit(query, k)
    for tau in (0, k - 1):
        pos, dist = ho.hits(codes, k, sing, tau)
        assert int(pos[-1]) == n and int(dist[-1]) == 0
        assert tau == 0 or (int(pos[0]) == 1 and int(dist[0]) == k - 1)
        for got in (free.kmer_edist_hits(_ascii(codes), k, query, tau, with_dist=True), free.kmer_edist_hits_packed(po.pack_codes(codes), n, k, query, tau, with_dist=True),
                    free.kmer_pattern_edist_hits(_ascii(codes), k, sing, tau, with_dist=True),
                    free.kmer_pattern_edist_hits_packed(po.pack_codes(codes), n, k, sing, tau, with_dist=True)):
            assert np.array_equal(got[0], pos) and np.array_equal(got[1], dist)


def test_patterns_with_n_an_empty_set_and_singletons():
    free = _free()
    rng = np.random.default_rng(0x9A9)
    for k, n in ((1, 20), (12, 80), (23, 150), (32, 200)):
        codes = rng.integers(0, 4, size=n)
        s, words = _ascii(codes, rng), po.pack_codes(codes, junk=0x123456789ABCDEF0)
        all_n = po.from_iupac("N" * k)
        assert np.array_equal(free.kmer_pattern_edist_hits(s, k, all_n, 0), np.arange(k, n + 1))  # all-N: every end from k on at distance 0
        sets = po.random_sets(rng, k)
        with_n = po.from_sets([{0, 1, 2, 3} if i % 3 == 0 else x for i, x in enumerate(sets)])
        empty = po.from_sets([set() if i == k // 2 else x for i, x in enumerate(sets)])  # an empty set never matches
        none = po.from_sets([set()] * k)
        for pat in (with_n, empty, none, "ACGTRYKMSWBDHVNN"[:k] if k <= 16 else None):
            if pat is None:
                continue
            p = po.from_iupac(pat) if isinstance(pat, str) else pat
            for tau in (0, 2, k - 1, k):
                want = ho.hits(codes, k, p, tau)
                for got in (free.kmer_pattern_edist_hits(s, k, pat, tau, with_dist=True), free.kmer_pattern_edist_hits_packed(words, n, k, pat, tau, with_dist=True)):
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, tau)
                assert want[0].size == _count1("ascii", s, n, k, p, tau, pattern=True)
        assert free.kmer_pattern_edist_hits(s, k, none, k - 1).size == 0 and free.kmer_pattern_edist_hits(s, k, none, k).size == n


def test_no_windows_and_the_fill():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()
    w = np.zeros(1, dtype=np.uint64)
    for k in (0, 7):  # k == 0, n < k: the family's rule, although E(j) is defined for n < k
        for form, src in (("ascii", s), ("packed", w)):
            for pattern, q in ((False, 5), (True, po.from_2bit(5, 3))):
                st, _, o = _hits(form, src, 6, k, q, 40, 4, pattern)
                assert st == L.OK and o.read()[0] == 0 and (o.w == FILL64).all() and (o.d == 0x5A).all()
    assert ho.hits(np.zeros(6, dtype=int), 7, po.from_2bit(0, 7), 9)[0].size == 0
    free = _free()
    assert free.kmer_edist_hits(s, 7, 0, 9).size == 0 and free.kmer_edist_hits_packed(w, 6, 0, 0, 9).size == 0


def test_invalid_byte_its_index_and_untouched_outputs():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(14)
    k, n = 7, 90
    query = int(ro.random_queries(rng, 1, k)[0])
    s = _ascii(rng.integers(0, 4, size=n), rng)
    for at in ((n - 1,), (0,), (40, 17), (88, 3)):  # the last byte, the first, two: the smaller index
        t = s.copy()
        for i, a in enumerate(at):
            t[a] = (ord("N"), ord("x"))[i]
        first = min(at)
        for pattern, q in ((False, query), (True, po.from_2bit(query, k))):
            for cap in (0, 5):
                st, e, o = _hits("ascii", t, n, k, q, k, cap, pattern)
                assert st == L.INVALID_BASE and (e.byte, e.index) == (int(t[first]), first) and o.untouched()
        with pytest.raises(bn.NucleotideError) as ei:
            free.kmer_edist_hits(t, k, query, 2)
        assert (ei.value.byte, ei.value.index) == (int(t[first]), first)


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(9, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    pat = np.zeros(8, dtype=np.uint32)
    for kind in ("", "pattern_"):
        f = {name: getattr(lib, f"bitnuc_kmer_{kind}edist_{name}") for name in ("hits", "hits_packed", "hits_async", "hits_packed_async")}
        good_q = C.c_void_p(pat.ctypes.data) if kind else C.c_uint64(0)

        def call(name, src, n, k, q, end, cap, n_hits, n_words=9):
            head = (src, n_words, n) if "packed" in name else (src, n)
            err = L.BitnucErr()
            st = f[name](None, *head, k, q, 3, end, None, cap, C.cast(n_hits, C.POINTER(C.c_uint64)) if not name.endswith("_async") else n_hits, C.byref(err))
            return st, err

        o = Out(8)
        bad_q = None if kind else C.c_uint64(0)  # a NULL pattern; an exact query is a value and cannot be wrong
        for name in f:
            src = wp if "packed" in name else sp
            if name.endswith("_async"):
                # 1. the _async forms check the context first, whatever else is wrong
                st, e = call(name, None, 2**40, 40, bad_q, None, 9, None, n_words=0)
                assert st == L.UNSUPPORTED and e.value == 0, name
                continue
            # 2. k > 32, with everything else wrong too
            st, e = call(name, None, 2**40, 33, bad_q, None, 9, None, n_words=0)
            assert st == L.SEQUENCE_TOO_LONG and e.value == 33, name
            # 3. packed: too few words, before the pattern and the outputs
            if "packed" in name:
                st, e = call(name, None, 289, 5, bad_q, None, 9, None)
                assert st == L.INVALID_LENGTH and e.value == 289, name
            # 4. the pattern (NULL, or not 4-byte aligned), before the outputs
            if kind:
                for q in (None, C.c_void_p(pat.ctypes.data + 2)):
                    st, e = call(name, None, 3, 5, q, None, 9, None)
                    assert st == L.UNSUPPORTED and e.value == 0, name
            # 5. the outputs (check_hits_out), before the no-windows case (n 3 < k 5) and the reference
            for end, cap, n_hits in ((o.wp(), 8, None), (o.wp(), 8, C.c_void_p(o.np_().value + 4)), (None, 1, o.np_()), (C.c_void_p(o.wp().value + 4), 8, o.np_())):
                st, e = call(name, None, 3, 5, good_q, end, cap, n_hits)
                assert st == L.UNSUPPORTED and e.value == 0, (name, end, cap, n_hits)
            assert o.untouched()
            # 6. no windows: *n_hits = 0 and nothing else, before the reference is looked at (NULL)
            for k, n in ((0, 100), (6, 5)):
                o2 = Out(8)
                st, _ = call(name, None, n, k, good_q, o2.wp(), 8, o2.np_())
                assert st == L.OK and o2.read()[0] == 0 and (o2.w == FILL64).all(), name
            # 7. then a NULL reference, or packed words not 8-byte aligned
            st, _ = call(name, None, 64, 5, good_q, o.wp(), 8, o.np_())
            assert st == L.UNSUPPORTED, name
            if "packed" in name:
                st, _ = call(name, C.c_void_p(words.ctypes.data + 4), 64, 5, good_q, o.wp(), 8, o.np_())
                assert st == L.UNSUPPORTED, name
            assert o.untouched()
            # cap == 0 with end == NULL is valid: the count only
            o2 = Out(0)
            st, _ = call(name, src, 256, 5, good_q, None, 0, o2.np_())
            assert st == L.OK and o2.read()[0] == ho.hits(np.tile([0, 1, 2, 3], 64) if "packed" not in name else np.zeros(256, dtype=int), 5,
                                                         np.zeros(4, dtype=np.uint32) if kind else po.from_2bit(0, 5), 3)[0].size, name


def test_host_cutoff_is_judged_on_n():
    """Below the cutoff (1 Mi ends, one query) the host forms need no context; at it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    k = 16
    codes = np.random.default_rng(1).integers(0, 4, size=2**20)
    s, w = _ascii(codes), po.pack_codes(codes)
    for n, host in ((2**20 - 1, True), (2**20, False)):
        for form, src in (("ascii", s[:n]), ("packed", w)):
            for pattern, q in ((False, 12345), (True, po.from_2bit(12345, k))):
                st, _, o = _hits(form, src, n, k, q, 1, 4, pattern)
                assert st == (L.OK if host else L.UNSUPPORTED), (n, form)
                assert host or o.untouched()
