"""CPU tests of the indel-tolerant k-mer search along a reference (bitnuc_kmer_edist_best / _count_multi, their _packed forms and the pattern twins):
the host path below the cutoff, through a NULL context, against tests/kmer_edist_oracle.py (the plain DP; the host path is the bit-parallel recurrence)
-- every k in 1 .. 32 at n in {k, k + 1, 2k, 63, 64, 65, 200}; planted copies with one deletion, one insertion, one substitution and two mixed edits,
(dist, end) asserted by hand; ties between two ends; an exact occurrence; an all-N pattern, a pattern with an empty set, singleton patterns equal to
the exact forms; dist <= the Hamming best match's and counts >= the Hamming count's; tau in {0, 1, k - 1, k, 2^32 - 1}, monotone in tau; fills and zeros
for k == 0, n < k and n_queries == 0; an invalid byte with its index and the outputs untouched; packed junk above 2n; the argument checks in their
documented order; guard words and bytes around every output with dist at an odd offset; the host helpers (csrc/kmer_edist_host.h) under ASan + UBSan
in a stand-alone program (tests/c/kmer_edist_host_sanitize.cpp).  Every comparison is exact.  (The bitnuc.hpp mirror, tests/cpp/test_kmer_edist_hpp.cpp,
needs a context and runs from tests/test_gpu_kmer_edist.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_edist_oracle as ko
import pattern_oracle as po
import reads_best_oracle as ro
import reads_edist_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL64 = 0x5A5A5A5A5A5A5A5A
NO_END = 2**64 - 1


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


def _ascii(codes, rng=None):
    s = ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)
    if rng is not None:
        s[rng.random(s.size) < 0.3] |= 0x20  # about 30 % lowercase
    return s


class Out:
    """end / counts (u64) inside GUARD guard words, dist (u8) at byte offset 1 of its buffer"""

    def __init__(self, nq):
        self.nq = nq
        self.w = np.full(nq + 2 * GUARD, FILL64, dtype=np.uint64)
        self.d = np.full(1 + nq + GUARD, 0x5A, dtype=np.uint8)

    def wp(self):
        return C.c_void_p(self.w.ctypes.data + 8 * GUARD)

    def dp(self):
        return C.c_void_p(self.d.ctypes.data + 1)

    def untouched(self):
        return bool((self.w == FILL64).all() and (self.d == 0x5A).all())

    def read(self):
        n = self.nq
        assert (self.w[:GUARD] == FILL64).all() and (self.w[GUARD + n:] == FILL64).all(), "end / counts written outside [0, n_queries)"
        assert (self.d[:1] == 0x5A).all() and (self.d[1 + n:] == 0x5A).all(), "dist written outside [0, n_queries)"
        return self.w[GUARD:GUARD + n].copy(), self.d[1:1 + n].copy()


def _queries(queries, pattern):
    q = ko.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    return q, q.shape[0]


def _src(form, src, n):
    head = (C.c_void_p(src.ctypes.data) if src is not None and src.size else None,)
    return head + ((src.size if src is not None else 0, n) if form == "packed" else (n,))


def _best(form, src, n, k, queries, pattern=False):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    fn = getattr(L.load(), "bitnuc_kmer_" + ("pattern_" if pattern else "") + "edist_best" + ("" if form == "ascii" else "_packed"))
    q, nq = _queries(queries, pattern)
    o = Out(nq)
    st, e = _raw(fn, None, *_src(form, src, n), k, C.c_void_p(q.ctypes.data) if nq else None, nq, o.wp(), o.dp())
    return st, e, o


def _count(form, src, n, k, queries, taus, pattern=False):
    from bitnuc_amd import _lib as L
    fn = getattr(L.load(), "bitnuc_kmer_" + ("pattern_" if pattern else "") + "edist_count_multi" + ("" if form == "ascii" else "_packed"))
    q, nq = _queries(queries, pattern)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(taus, dtype=np.uint32), (nq,)))
    o = Out(nq)
    st, e = _raw(fn, None, *_src(form, src, n), k, C.c_void_p(q.ctypes.data) if nq else None, C.c_void_p(t.ctypes.data) if nq else None, nq, o.wp())
    return st, e, o


def test_the_oracle_row_form_equals_the_three_term_recurrence():
    rng = np.random.default_rng(0x0AC1E)
    for _ in range(60):
        k = int(rng.integers(1, 33))
        n = int(rng.integers(0, 90))
        codes = rng.integers(0, 4, size=n)
        p = po.from_sets(po.random_sets(rng, k)) if rng.integers(0, 2) else po.from_2bit(int(rng.integers(0, 2**63)), k)
        if n > k and rng.integers(0, 2):
            c = eo.plant(rng, rng.integers(0, 4, size=k), 2)[:n]
            codes[:len(c)] = c
        assert np.array_equal(ko.ends(codes, k, p), ko.ends_three_term(codes, k, p))


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "kmer_edist_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "kmer edist host ok" in out.stdout


@pytest.mark.parametrize("k0", [1, 9, 17, 25])
def test_host_path_against_the_dp(k0):
    """k = k0 .. k0 + 7 (1 .. 32 over the four cases) at n in {k, k + 1, 2k, 63, 64, 65, 200}; both layouts, both query kinds, both outputs"""
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0xED17 + k0)
    for k in range(k0, k0 + 8):
        for n in sorted({k, k + 1, 2 * k, 63, 64, 65, 200}):
            if n < k:
                continue
            nq = [1, 2, 5][(k + n) % 3]
            queries = ro.random_queries(rng, nq, k)
            codes = rng.integers(0, 4, size=n)
            for q in range(nq):  # a copy of every query with up to 3 edits, where it fits
                c = eo.plant(rng, ro.query_codes(queries[q], k), int(rng.integers(0, 4)))[:n]
                at = int(rng.integers(0, n - len(c) + 1))
                codes[at:at + len(c)] = c
            s = _ascii(codes, rng)
            words = po.pack_codes(codes, junk=0xDEADBEEFDEADBEEF)  # junk above 2n
            sing = ko.singletons(queries, k)
            taus = rng.integers(0, k + 1, size=nq)
            end, dist, cnt = ko.kmer_edist_both(codes, k, sing, taus)
            assert (end >= 1).all() and (end <= n).all() and (dist <= k).all()
            for form, src in (("ascii", s), ("packed", words)):
                for pattern, qq in ((False, queries), (True, sing)):
                    st, _, o = _best(form, src, n, k, qq, pattern)
                    got = o.read()
                    assert st == L.OK and np.array_equal(got[0], end) and np.array_equal(got[1], dist), (form, pattern, k, n)
                    st, _, o = _count(form, src, n, k, qq, taus, pattern)
                    assert st == L.OK and np.array_equal(o.read()[0], cnt) and (o.d == 0x5A).all(), (form, pattern, k, n)
    free = _free()  # the numpy wrappers
    got = free.kmer_edist_best(s, k, queries)
    assert np.array_equal(got[0], end) and np.array_equal(got[1], dist) and got[0].dtype == np.uint64 and got[1].dtype == np.uint8
    got = free.kmer_edist_best_packed(words, n, k, queries)
    assert np.array_equal(got[0], end) and np.array_equal(got[1], dist)
    assert np.array_equal(free.kmer_edist_count_multi(s, k, queries, taus), cnt)
    assert np.array_equal(free.kmer_edist_count_multi_packed(words, n, k, queries, taus), cnt)
    got = free.kmer_pattern_edist_best(s, k, sing)
    assert np.array_equal(got[0], end) and np.array_equal(got[1], dist)
    got = free.kmer_pattern_edist_best_packed(words, n, k, sing)
    assert np.array_equal(got[0], end) and np.array_equal(got[1], dist)
    assert np.array_equal(free.kmer_pattern_edist_count_multi(s, k, sing, taus), cnt)
    assert np.array_equal(free.kmer_pattern_edist_count_multi_packed(words, n, k, sing, taus), cnt)


def test_planted_indels_by_hand():
    """reads_edist_oracle.planted_cases' five reads, each taken as a reference of its own: the planted copy starts at base 14, so its end is 14 + its
    length; the Hamming best match sees about half of the bases behind an indel differ"""
    free = _free()
    k, read_len, _, _, s, queries = eo.planted_cases()
    sing = ko.singletons(queries, k)
    for r, (d, e) in enumerate(((1, 14 + 15), (1, 14 + 17), (1, 14 + 16), (2, 14 + 16), (0, 14 + 16))):
        ref = s[r * read_len:(r + 1) * read_len]
        codes = ro.codes_of(ref)
        end, dist = ko.kmer_edist_best(codes, k, sing)
        assert (int(dist[1]), int(end[1])) == (d, e)
        words = po.pack_codes(codes, junk=2**64 - 1)
        for got in (free.kmer_edist_best(ref, k, queries), free.kmer_edist_best_packed(words, read_len, k, queries),
                    free.kmer_pattern_edist_best(ref, k, sing), free.kmer_pattern_edist_best_packed(words, read_len, k, sing)):
            assert np.array_equal(got[0], end) and np.array_equal(got[1], dist), r
        ham = free.kmer_hdist_best(ref, k, queries)
        assert (dist <= ham[1]).all() and (r >= 2 or ham[1][1] > 4)
        # the ends at distance <= 1 of the planted copy: the count sees the neighbours of the best end too
        cnt = free.kmer_edist_count_multi(ref, k, queries, [k, d])
        assert int(cnt[0]) == read_len and cnt[1] == ko.count(ko.ends(codes, k, sing[1]), d) and cnt[1] >= 1


def test_ties_the_smallest_end_and_an_exact_occurrence():
    free = _free()
    k, n = 6, 40
    q = np.array([0, 1, 2, 3, 1, 0])
    codes = np.full(n, 2)
    codes[5:11], codes[20:26] = q, q  # the same distance at two ends: the smaller one, the first occurrence
    far = ro.word_of([3] * k)
    queries = np.array([far, ro.word_of(q) | (1 << 40)], dtype=np.uint64)  # junk above 2k
    end, dist = free.kmer_edist_best(_ascii(codes), k, queries)
    assert (int(end[1]), int(dist[1])) == (11, 0)
    assert (int(end[0]), int(dist[0])) == (9, k - 1)  # TTTTTT: the one T of the sequence, at base 9, matches one position
    want = ko.kmer_edist_best(codes, k, ko.singletons(queries, k))
    assert np.array_equal(end, want[0]) and np.array_equal(dist, want[1])
    near = q.copy()
    near[2] = 0  # one substitution away from both copies
    end, dist = free.kmer_edist_best_packed(po.pack_codes(codes), n, k, [ro.word_of(near)])
    assert (int(end[0]), int(dist[0])) == (11, 1)
    assert list(free.kmer_edist_count_multi(_ascii(codes), k, [ro.word_of(q)], 0)) == [2]


def test_patterns_all_n_empty_set_and_singletons():
    free = _free()
    rng = np.random.default_rng(0x9A8)
    for k, n in ((1, 20), (12, 50), (32, 150)):
        codes = rng.integers(0, 4, size=n)
        s, words = _ascii(codes, rng), po.pack_codes(codes, junk=0x123456789ABCDEF0)
        all_n = po.from_iupac("N" * k)
        end, dist = free.kmer_pattern_edist_best(s, k, [all_n])
        assert (int(end[0]), int(dist[0])) == (k, 0)  # all-N: dist 0 at end k
        assert list(free.kmer_pattern_edist_count_multi(s, k, [all_n], 0)) == [n - k + 1]
        sets = [po.random_sets(rng, k) for _ in range(4)]
        sets[2] = [set() if i == k // 2 else x for i, x in enumerate(sets[2])]  # an empty set never matches
        pats = ko.as_patterns([po.from_sets(x) for x in sets] + [po.from_sets([set()] * k)])
        taus = rng.integers(0, k + 1, size=5)
        want = ko.kmer_edist_both(codes, k, pats, taus)
        assert (int(want[0][4]), int(want[1][4])) == (1, k)  # every set empty
        for got in (free.kmer_pattern_edist_best(s, k, pats), free.kmer_pattern_edist_best_packed(words, n, k, pats)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
        assert np.array_equal(free.kmer_pattern_edist_count_multi(s, k, pats, taus), want[2])
        assert np.array_equal(free.kmer_pattern_edist_count_multi_packed(words, n, k, pats, taus), want[2])


def test_never_above_the_hamming_forms_and_the_count_in_tau():
    free = _free()
    rng = np.random.default_rng(0xBEF)
    for k, n in ((16, 3000), (31, 2000), (5, 300), (1, 40)):
        queries = ro.random_queries(rng, 6, k)
        codes = rng.integers(0, 4, size=n)
        for q in range(6):
            c = eo.plant(rng, ro.query_codes(queries[q], k), q % 4)
            at = int(rng.integers(0, n - len(c) + 1))
            codes[at:at + len(c)] = c
        s = _ascii(codes, rng)
        sing = ko.singletons(queries, k)
        end, dist = free.kmer_edist_best(s, k, queries)
        assert (dist <= free.kmer_hdist_best(s, k, queries)[1]).all()
        last = None
        for tau in sorted({0, 1, k - 1, k, 2**32 - 1}):
            cnt = free.kmer_edist_count_multi(s, k, queries, tau)
            assert np.array_equal(cnt, ko.kmer_edist_count(codes, k, sing, tau)), (k, tau)
            assert (cnt >= free.kmer_hdist_count_multi(s, k, queries, tau)).all()
            assert last is None or (cnt >= last).all()  # monotone in tau
            if tau >= k:
                assert (cnt == n).all()  # tau >= k counts every end
            last = cnt
        assert np.array_equal(free.kmer_edist_count_multi(s, k, queries, dist.astype(np.int64)) >= 1, np.ones(6, dtype=bool))


def test_fills_and_zeros_without_windows_and_without_queries():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()
    w = np.zeros(1, dtype=np.uint64)
    for k, queries in ((0, [1, 2]), (7, [1, 2])):  # k == 0, n < k: the family's rule, although E(j) is defined for n < k
        for form, src in (("ascii", s), ("packed", w)):
            for pattern in (False, True):
                qq = ko.singletons(queries, 3) if pattern else queries
                st, _, o = _best(form, src, 6, k, qq, pattern)
                got = o.read()
                assert st == L.OK and (got[0] == NO_END).all() and (got[1] == 0xFF).all()
                st, _, o = _count(form, src, 6, k, qq, 5, pattern)
                assert st == L.OK and (o.read()[0] == 0).all()
    for form, src in (("ascii", s), ("packed", w)):  # n_queries == 0: nothing written
        st, _, o = _best(form, src, 6, 3, [])
        assert st == L.OK and o.untouched()
        st, _, o = _count(form, src, 6, 3, [], 1)
        assert st == L.OK and o.untouched()
    assert not ko.has_windows(6, 0) and not ko.has_windows(6, 7) and ko.kmer_edist_count(np.zeros(6, dtype=int), 7, ko.singletons([1], 7), 9)[0] == 0


def test_invalid_byte_its_index_and_untouched_outputs():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(13)
    k, n = 7, 90
    queries = ro.random_queries(rng, 3, k)
    s = _ascii(rng.integers(0, 4, size=n), rng)
    for at in ((n - 1,), (0,), (40, 17), (88, 3)):  # the last byte, the first, two: the smaller index
        t = s.copy()
        for i, a in enumerate(at):
            t[a] = (ord("N"), ord("x"))[i]
        first = min(at)
        for pattern, qq in ((False, queries), (True, ko.singletons(queries, k))):
            st, e, o = _best("ascii", t, n, k, qq, pattern)
            assert st == L.INVALID_BASE and (e.byte, e.index) == (int(t[first]), first) and o.untouched()
            st, e, o = _count("ascii", t, n, k, qq, 2, pattern)
            assert st == L.INVALID_BASE and (e.byte, e.index) == (int(t[first]), first) and o.untouched()
        with pytest.raises(bn.NucleotideError) as ei:
            free.kmer_edist_best(t, k, queries)
        assert (ei.value.byte, ei.value.index) == (int(t[first]), first)


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = C.c_void_p(s.ctypes.data)
    words = np.zeros(9, dtype=np.uint64)
    wp = C.c_void_p(words.ctypes.data)
    q = np.zeros(32, dtype=np.uint64)  # eight patterns as well (all sets empty)
    qp = C.c_void_p(q.ctypes.data)
    t = np.zeros(33, dtype=np.uint32)
    tp = C.c_void_p(t.ctypes.data)
    for kind, qalign in (("", 4), ("pattern_", 2)):  # a pointer that breaks the kind's alignment: 8 bytes exact, 4 bytes patterns
        f = {name: getattr(lib, f"bitnuc_kmer_{kind}edist_{name}") for name in ("best", "best_packed", "best_async", "best_packed_async", "count_multi",
                                                                                "count_multi_packed", "count_multi_async", "count_multi_packed_async")}

        def call(name, src, n, k, queries, nq, out, extra=None, n_words=9):
            head = (src, n_words, n) if "packed" in name else (src, n)
            mid = (queries, nq, out, extra) if name.startswith("best") else (queries, extra, nq, out)
            return _raw(f[name], None, *head, k, *mid)

        o = Out(8)
        for name in f:
            best = name.startswith("best")
            src = wp if "packed" in name else sp
            ex = o.dp() if best else tp
            if name.endswith("_async"):
                # 1. the _async forms check the context first, whatever else is wrong
                st, e = call(name, None, 2**40, 40, None, 70000, None, None, n_words=0)
                assert st == L.UNSUPPORTED and e.value == 0, name
                continue
            # 2. k > 32, with everything else wrong too
            st, e = call(name, None, 2**40, 33, None, 70000, None, None, n_words=0)
            assert st == L.SEQUENCE_TOO_LONG and e.value == 33, name
            # 3. packed: too few words
            if "packed" in name:
                st, e = call(name, None, 289, 5, None, 70000, None, None)
                assert st == L.INVALID_LENGTH and e.value == 289, name
            # 4. n_queries == 0: OK, nothing written, even with NULL arrays
            st, e = call(name, None, 256, 5, None, 0, None, None)
            assert st == L.OK, name
            # 5. too many queries, before the arrays
            st, e = call(name, None, 256, 5, None, 65537, None, None)
            assert st == L.UNSUPPORTED and e.value == 65537, name
            # 6. the arrays, before the no-windows case (n 3 < k 5) and the reference
            bad = [(None, o.wp(), ex), (C.c_void_p(q.ctypes.data + qalign), o.wp(), ex), (qp, None, ex), (qp, C.c_void_p(o.wp().value + 4), ex), (qp, o.wp(), None)]
            if not best:
                bad.append((qp, o.wp(), C.c_void_p(t.ctypes.data + 2)))
            for qq, out, extra in bad:
                st, e = call(name, None, 3, 5, qq, 8, out, extra)
                assert st == L.UNSUPPORTED and e.value == 0, (name, qq, out, extra)
            assert o.untouched()
            # 7. no windows: the fill / zeros in [0, n_queries) and nothing after, before the reference is looked at (NULL); dist at an odd address
            for k, n in ((0, 100), (6, 5)):
                o2 = Out(8)
                st, _ = call(name, None, n, k, qp, 8, o2.wp(), o2.dp() if best else tp)
                got = o2.read()
                assert st == L.OK and ((got[0] == NO_END).all() and (got[1] == 0xFF).all() if best else (got[0] == 0).all() and (o2.d == 0x5A).all()), name
            # 8. then a NULL reference, or packed words not 8-byte aligned
            st, _ = call(name, None, 64, 5, qp, 8, o.wp(), ex)
            assert st == L.UNSUPPORTED, name
            if "packed" in name:
                st, _ = call(name, C.c_void_p(words.ctypes.data + 4), 64, 5, qp, 8, o.wp(), ex)
                assert st == L.UNSUPPORTED, name
            assert o.untouched()
            # and a valid call writes [0, n_queries) of each output only
            o2 = Out(3)
            st, _ = call(name, src, 256, 5, qp, 3, o2.wp(), o2.dp() if best else tp)
            assert st == L.OK and len(o2.read()[0]) == 3, name


def test_host_cutoff_is_judged_on_n_times_queries():
    """Below the cutoff (1 Mi end positions x queries) the host forms need no context; above it they do (a NULL context -> Unsupported)."""
    from bitnuc_amd import _lib as L
    n, k = 100000, 16  # x 10 < 2^20 <= x 11
    codes = np.random.default_rng(1).integers(0, 4, size=n)
    s, w = _ascii(codes), po.pack_codes(codes)
    for nq, host in ((10, True), (11, False)):
        for form, src in (("ascii", s), ("packed", w)):
            st, _, o = _best(form, src, n, k, np.arange(nq, dtype=np.uint64))
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            assert host or o.untouched()
            st, _, o = _count(form, src, n, k, np.arange(nq, dtype=np.uint64), 3)
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            assert host or o.untouched()
