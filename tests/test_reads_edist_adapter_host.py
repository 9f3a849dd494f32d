"""CPU tests of the 3' adapter per read (bitnuc_reads_edist_adapter / _packed / _batch / _batch_packed and the pattern twins): the host path below the cutoff,
through a NULL context, against tests/reads_edist_adapter_oracle.py (the plain DP over all rows with a direct Levenshtein minimum for the cut; the host path is
the bit-parallel walk with the last column kept) -- both layouts, both query kinds; k in {1, 2, 16, 31, 32} x lengths around k and the 64-base pieces x
min_overlap in {1, 3, k} x rates 0/1, 1/10, 1/5, 1/1; the planted reads of tests/reads_edist_adapter_cases.py with their five outputs asserted by hand; every
argument error with nothing written, in the header's order; invalid bytes with their absolute index (and none reported in a ragged read shorter than k);
fills; the header's identities; the oracle's cut against a naive Levenshtein per start; and the host helpers (csrc/reads_edist_adapter_host.h) under ASan +
UBSan in a stand-alone program (tests/c/reads_edist_adapter_host_sanitize.cpp).  Every comparison is exact equality of all five arrays; guard words and
bytes surround the outputs, both byte arrays start at odd offsets.  (The bitnuc.hpp mirror, tests/cpp/test_reads_edist_adapter_hpp.cpp, needs a context and
runs from tests/test_gpu_reads_edist_adapter.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_adapter_cases as cases
import reads_edist_adapter_oracle as ao
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
MAX_READ = 1 << 26  # BITNUC_EDIST_MAX_READ
RATES = [(0, 1), (1, 10), (1, 5), (1, 1)]
OK, INVALID_BASE, TOO_LONG, INVALID_RANGE, UNSUPPORTED = "BITNUC_OK", "BITNUC_INVALID_BASE", "BITNUC_SEQUENCE_TOO_LONG", "BITNUC_INVALID_RANGE", "BITNUC_UNSUPPORTED"


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _status(name):
    import re
    header = open(os.path.join(ROOT, "include", "bitnuc_hip.h")).read()
    return int(re.search(r"\b" + name + r"\s*=\s*(\d+)", header).group(1))


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


class Out:
    """the five outputs inside guarded host buffers: GUARD words around adapter / cut / end, overlap and dist at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(3)]
        self.d = [np.full(off + count + GUARD, 0x5A, dtype=np.uint8) for off in (1, 3)]

    def ptrs(self):
        return tuple(C.c_void_p(a.ctypes.data + 4 * GUARD) for a in self.w) + tuple(C.c_void_p(a.ctypes.data + off) for a, off in zip(self.d, (1, 3)))

    def untouched(self):
        return all((a == FILL32).all() for a in self.w) and all((a == 0x5A).all() for a in self.d)

    def read(self):
        n = self.count
        for a in self.w:
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "adapter / cut / end written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "overlap / dist written outside [0, count)"
        return tuple(a[GUARD:GUARD + n].copy() for a in self.w) + (self.d[0][1:1 + n].copy(), self.d[1][3:3 + n].copy())


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _queries(queries, pattern):
    q = rp.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    return q, q.shape[0]


def _call(name, *args, out=None, ptrs=None):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = getattr(L.load(), name)(None, *args, *(ptrs if ptrs is not None else out.ptrs()), C.byref(err))
    return st, err


def _fixed(form, s, read_len, count, k, queries, rule, pattern=False, words=None):
    """the raw fixed-layout entry point through a NULL context with guarded outputs: (status, err, Out)"""
    q, nq = _queries(queries, pattern)
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_adapter"
    o = Out(count)
    if form == "ascii":
        st, e = _call(name, _p(s), read_len, count, k, _p(q), nq, *rule, out=o)
    else:
        words = ro.pack_reads(s, read_len, count) if words is None else words
        st, e = _call(name + "_packed", _p(words), read_len, count, k, _p(q), nq, *rule, out=o)
    return st, e, o


def _ragged(form, s, off, k, queries, rule, pattern=False):
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count = off.size - 1
    q, nq = _queries(queries, pattern)
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_adapter_batch"
    o = Out(count)
    if form == "ascii":
        st, e = _call(name, _p(s), _p(off), count, k, _p(q), nq, *rule, out=o)
    else:
        words, woff = rb.pack_batch(s, off, seed=k), rb.word_offsets_of(off)  # (named: they must outlive the call)
        st, e = _call(name + "_packed", _p(words), _p(woff), _p(off), count, k, _p(q), nq, *rule, out=o)
    return st, e, o


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def _reads_with_adapters(rng, lens, k, queries, lower=True):
    """random reads of the given lengths; most reads of at least k bases carry a prefix of a query (sometimes whole, sometimes with one edit) at their end or,
    now and then, inside"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    s = _ascii(rng.integers(0, 4, int(off[-1])))
    for r, n in enumerate(lens):
        if n < k or rng.random() < 0.2:
            continue
        pre = [int(c) for c in ro.query_codes(queries[int(rng.integers(0, len(queries)))], k)][:int(rng.integers(1, k + 1))]
        if len(pre) > 3 and rng.random() < 0.5:
            x, how = int(rng.integers(0, len(pre))), int(rng.integers(0, 3))
            if how == 0:
                pre[x] = (pre[x] + 1) % 4
            elif how == 1:
                pre.insert(x, int(rng.integers(0, 4)))
            else:
                del pre[x]
        pre = pre[:n]
        at = n - len(pre) if rng.random() < 0.75 else int(rng.integers(0, n - len(pre) + 1))
        s[int(off[r]) + at:int(off[r]) + at + len(pre)] = _ascii(pre)
    if lower:
        s = np.where(rng.random(s.size) < 0.3, s | 0x20, s).astype(np.uint8)
    return s, off


def _random_queries(rng, nq):
    return rng.integers(0, 1 << 63, nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, nq, dtype=np.uint64)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_edist_adapter_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_oracle_cut_against_a_naive_levenshtein_per_start():
    """cut_of finds every start's distance in one DP of the reversed strings; here each start gets its own plain DP"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        i = int(rng.integers(1, 33))
        pattern = np.array([int(rng.integers(1, 1 << 32)) & ((1 << 32) - 1) for _ in range(4)], dtype=np.uint32) if rng.random() < 0.3 else \
            rp.singletons(_random_queries(rng, 1), 32)[0]
        sets = ao.sets_of(pattern, i)
        n = int(rng.integers(1, 80))
        t = rng.integers(0, 4, n)
        e = int(rng.integers(1, n + 1))
        w = min(e, 2 * i - 1)
        want = min((ao.lev(sets, t[s:e]), e - s) for s in range(e - w, e + 1))
        assert ao.cut_of(sets, t, e) == (want[0], e - want[1])


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_host_forms_against_the_oracle(k):
    """all eight host forms through a NULL context"""
    rng = np.random.default_rng(100 + k)
    for n in sorted({k, k + 1, 63, 64, 65, 127, 128, 129, 150} - set(range(k))):
        for mo in sorted({1, min(3, k), k}):
            num, den = RATES[int(rng.integers(0, 4))]
            count, nq = int(rng.integers(1, 7)), int(rng.integers(1, 6))
            queries = _random_queries(rng, nq)
            s, off = _reads_with_adapters(rng, [n] * count, k, queries)
            want = ao.reads_edist_adapter(s, n, count, k, queries, mo, num, den)
            rule = (mo, num, den)
            for pattern in (False, True):
                q = rp.singletons(queries, k) if pattern else queries
                for form in ("ascii", "packed"):
                    st, e, o = _fixed(form, s, n, count, k, q, rule, pattern)
                    assert st == _status(OK) and _same(o.read(), want), (k, n, mo, num, den, form, pattern)
                    st, e, o = _ragged(form, s, off, k, q, rule, pattern)
                    assert st == _status(OK) and _same(o.read(), want), (k, n, mo, num, den, form, pattern, "ragged")
    # every rate and overlap at one shape
    n, count = 70, 12
    queries = _random_queries(rng, 3)
    s, off = _reads_with_adapters(rng, [n] * count, k, queries)
    for num, den in RATES:
        for mo in sorted({1, min(3, k), k}):
            want = ao.reads_edist_adapter(s, n, count, k, queries, mo, num, den)
            for form in ("ascii", "packed"):
                st, e, o = _fixed(form, s, n, count, k, queries, (mo, num, den))
                assert st == _status(OK) and _same(o.read(), want), (k, mo, num, den, form)


@pytest.mark.parametrize("k", [2, 16, 32])
def test_ragged_lengths_and_real_patterns(k):
    """reads of 0, below k, k and around the pieces in one batch; patterns with sets of several bases and an empty set"""
    rng = np.random.default_rng(200 + k)
    lens = [0, k - 1, k, k + 1, 5, 63, 64, 65, 0, 127, 128, 129, 150, 1, 33]
    queries = _random_queries(rng, 4)
    s, off = _reads_with_adapters(rng, lens, k, queries)
    pats = rp.singletons(queries, k).copy()
    pats[1, :] |= np.uint32(1 << (k // 2))         # position k / 2 of pattern 1: any base
    pats[2, :] &= np.uint32(~np.uint32(1 << (k - 1)))  # the last position of pattern 2: the empty set
    for num, den in RATES:
        for mo in sorted({1, min(3, k), k}):
            for form in ("ascii", "packed"):
                want = ao.reads_edist_adapter_batch(s, off, k, queries, mo, num, den)
                st, e, o = _ragged(form, s, off, k, queries, (mo, num, den))
                assert st == _status(OK) and _same(o.read(), want), (k, mo, num, den, form)
                want = ao.reads_pattern_edist_adapter_batch(s, off, k, pats, mo, num, den)
                st, e, o = _ragged(form, s, off, k, pats, (mo, num, den), pattern=True)
                assert st == _status(OK) and _same(o.read(), want), (k, mo, num, den, form, "patterns")


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_planted_reads_by_hand(case):
    name, reads, adapters, mo, num, den, want = case
    s, queries = cases.arrays(reads, adapters)
    want = cases.want_arrays(want)
    assert _same(ao.reads_edist_adapter(s, cases.N, len(reads), cases.K, queries, mo, num, den), want), "the hand-made expectation and the oracle disagree"
    off = np.arange(len(reads) + 1, dtype=np.uint64) * cases.N
    for form in ("ascii", "packed"):
        st, e, o = _fixed(form, s, cases.N, len(reads), cases.K, queries, (mo, num, den))
        assert st == _status(OK) and _same(o.read(), want), form
        st, e, o = _ragged(form, s, off, cases.K, queries, (mo, num, den))
        assert st == _status(OK) and _same(o.read(), want), form


def test_planted_reads_at_every_rate():
    for name, reads, adapters, mo, _, _, _ in cases.CASES:
        s, queries = cases.arrays(reads, adapters)
        for num, den in RATES:
            want = ao.reads_edist_adapter(s, cases.N, len(reads), cases.K, queries, mo, num, den)
            for form in ("ascii", "packed"):
                st, e, o = _fixed(form, s, cases.N, len(reads), cases.K, queries, (mo, num, den))
                assert st == _status(OK) and _same(o.read(), want), (name, num, den, form)


def test_python_methods_and_identities():
    """the eight api methods (NULL context below the cutoff); identity 1 (min_overlap = k, rate 1/1: the whole-read best match and its start), identity 2
    (rate 0/1, min_overlap 1: plain string matching), 3 (singleton patterns), 4 (ragged on equal lengths), 5 (dist is the Levenshtein distance of the prefix
    to read[cut:end]) and 6 (ASCII and packed agree)"""
    from bitnuc_amd import api
    ctx = api.context_free()
    rng = np.random.default_rng(9)
    k, n, count = 16, 90, 40
    queries = _random_queries(rng, 5)
    s, off = _reads_with_adapters(rng, [n] * count, k, queries)
    words, woff = ro.pack_reads(s, n, count), np.arange(count + 1, dtype=np.uint64) * ((n + 31) // 32)
    pats = rp.singletons(queries, k)
    for mo, num, den in ((3, 1, 10), (k, 1, 1), (1, 0, 1), (1, 1, 5)):
        want = ao.reads_edist_adapter(s, n, count, k, queries, mo, num, den)
        got = [ctx.reads_edist_adapter(s, n, k, queries, mo, num, den), ctx.reads_edist_adapter_packed(words, n, count, k, queries, mo, num, den),
               ctx.reads_pattern_edist_adapter(s, n, k, pats, mo, num, den), ctx.reads_pattern_edist_adapter_packed(words, n, count, k, pats, mo, num, den),
               ctx.reads_edist_adapter_batch(s, off, k, queries, mo, num, den), ctx.reads_edist_adapter_batch_packed(words, woff, off, k, queries, mo, num, den),
               ctx.reads_pattern_edist_adapter_batch(s, off, k, pats, mo, num, den),
               ctx.reads_pattern_edist_adapter_batch_packed(words, woff, off, k, pats, mo, num, den)]
        for i, g in enumerate(got):
            assert _same(g, want), (mo, num, den, i)
        adapter, cut, end, overlap, dist = want
        hit = adapter != ao.NO_U32
        assert hit.any()
        codes = ro.codes_of(s).reshape(count, n)
        for r in np.nonzero(hit)[0]:  # identity 5
            assert ao.lev(ao.sets_of(pats[adapter[r]], int(overlap[r])), codes[r, cut[r]:end[r]]) == dist[r]
        if (mo, num, den) == (k, 1, 1):  # identity 1
            bq, be, bd = ctx.reads_edist_best(s, n, k, queries, second=False)
            assert np.array_equal(adapter, bq) and np.array_equal(end, be) and np.array_equal(dist, bd) and (overlap == k).all()
            start, sd = ctx.reads_edist_start(s, n, k, queries, bq, be, "start", 0)
            assert np.array_equal(cut, start) and np.array_equal(dist, sd)
        if (mo, num, den) == (1, 0, 1):  # identity 2
            text = bytes(s & 0xDF).decode()
            for r in range(count):
                read = text[r * n:(r + 1) * n]
                found = None
                for q in range(len(queries)):
                    a = "".join("ACGT"[c] for c in ro.query_codes(queries[q], k))
                    at = read.find(a)
                    cand = (0, q, at + k, k) if at >= 0 else max(((k - i, q, n, i) for i in range(1, k) if read.endswith(a[:i])), key=lambda c: c[3], default=None)
                    if cand is not None and (found is None or cand < found):
                        found = cand
                if found is None:
                    assert adapter[r] == ao.NO_U32
                else:
                    assert (adapter[r], end[r], overlap[r], dist[r], cut[r]) == (found[1], found[2], found[3], 0, found[2] - found[3]), r


def test_fills():
    rng = np.random.default_rng(3)
    s = _ascii(rng.integers(0, 4, 200))
    q = _random_queries(rng, 2)
    fill = ao.fill5(5)
    for form in ("ascii", "packed"):
        for args in ((s, 40, 5, 0, q), (s, 40, 5, 16, q[:0]), (s, 10, 5, 16, q)):  # k == 0 (the rule is not judged), no queries, read_len < k
            st, e, o = _fixed(form, *args, (0 if args[3] == 0 else 3, 1, 10))
            assert st == _status(OK) and _same(o.read(), fill), (form, args[1:4])
        off = np.array([0, 3, 3, 10, 25, 25], dtype=np.uint64)  # every read shorter than k = 16
        st, e, o = _ragged(form, s, off, 16, q, (3, 1, 10))
        assert st == _status(OK) and _same(o.read(), fill), form
    # nothing admissible: rate 0 / 1 on reads without an exact copy of a prefix of three
    s = np.frombuffer(b"C" * 80, dtype=np.uint8)
    st, e, o = _fixed("ascii", s, 40, 2, 16, np.array([0], dtype=np.uint64) + np.uint64(0xAAAAAAAA), (3, 0, 1))  # the adapter is all G
    assert st == _status(OK) and _same(o.read(), ao.fill5(2))


def test_argument_errors_in_order_and_nothing_written():
    rng = np.random.default_rng(4)
    s = _ascii(rng.integers(0, 4, 400))
    words = ro.pack_reads(s, 40, 10)
    q = _random_queries(rng, 2)
    off = np.arange(11, dtype=np.uint64) * 40
    woff = np.arange(11, dtype=np.uint64) * 2
    TL, UN, IR = _status(TOO_LONG), _status(UNSUPPORTED), _status(INVALID_RANGE)

    def fixed(name, data, read_len, count, k, queries, nq, rule, ptrs=None):
        o = Out(max(count, 1) if count < 1000 else 1)
        st, e = _call(name, _p(data), read_len, count, k, _p(queries) if queries is not None else None, nq, *rule, out=o, ptrs=ptrs(o) if ptrs else None)
        assert o.untouched(), name
        return st, e.value

    for name, data in (("bitnuc_reads_edist_adapter", s), ("bitnuc_reads_edist_adapter_packed", words)):
        assert fixed(name, data, 40, 10, 33, q, 2, (0, 5, 0)) == (TL, 33)                      # k first, whatever the rule is
        assert fixed(name, data, 0xFFFFFFFF, 10, 16, q, 2, (0, 5, 0)) == (UN, 0xFFFFFFFF)      # then the layout's sizes
        assert fixed(name, data, 40, 10, 16, q, 65537, (0, 5, 0)) == (UN, 65537)               # then the query limit
        assert fixed(name, data, 40, 10, 16, q, 2, (0, 5, 0)) == (UN, 0)                       # min_overlap == 0
        assert fixed(name, data, 40, 10, 16, q, 2, (17, 5, 0)) == (UN, 17)                     # min_overlap > k
        assert fixed(name, data, 40, 10, 16, q, 2, (3, 5, 0)) == (UN, 5)                       # err_den == 0
        assert fixed(name, data, 40, 10, 16, q, 2, (3, 11, 10)) == (UN, 11)                    # err_num > err_den
        assert fixed(name, data, MAX_READ + 1, 1, 16, q, 2, (3, 11, 10)) == (UN, 11)           # the rule before the read length
        assert fixed(name, data, MAX_READ + 1, 1, 16, q, 2, (3, 1, 10)) == (UN, MAX_READ + 1)
        assert fixed(name, data, MAX_READ + 1, 0, 16, q, 2, (3, 1, 10)) == (UN, MAX_READ + 1)  # ... before count == 0
        assert fixed(name, None, 40, 0, 16, None, 2, (3, 1, 10), ptrs=lambda o: (None,) * 5)[0] == _status(OK)  # count == 0: no pointer is looked at
        for drop in range(5):                                                                  # every output is required
            assert fixed(name, data, 40, 10, 16, q, 2, (3, 1, 10), ptrs=lambda o: tuple(None if i == drop else p for i, p in enumerate(o.ptrs())))[0] == UN
        for odd in range(3):                                                                   # adapter, cut, end: 4-byte aligned
            assert fixed(name, data, 40, 10, 16, q, 2, (3, 1, 10),
                         ptrs=lambda o: tuple(C.c_void_p(p.value + 2) if i == odd else p for i, p in enumerate(o.ptrs())))[0] == UN
        assert fixed(name, data, 40, 10, 16, None, 2, (3, 1, 10))[0] == UN                     # queries NULL with n_queries > 0
        assert fixed(name, None, 40, 10, 16, q, 2, (3, 1, 10))[0] == UN                        # no reads
    # ragged: the tables' own checks, then the read length limit, before the data pointer
    o = Out(10)
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    st, e = _call("bitnuc_reads_edist_adapter_batch", _p(s), _p(bad_off), 10, 16, _p(q), 2, 3, 1, 10, out=o)
    assert st == IR and o.untouched()
    st, e = _call("bitnuc_reads_edist_adapter_batch", _p(s), None, 10, 16, _p(q), 2, 3, 1, 10, out=o)
    assert st == UN and o.untouched()
    long_off = np.array([0, 5, 5 + MAX_READ + 1], dtype=np.uint64)
    st, e = _call("bitnuc_reads_edist_adapter_batch", None, _p(long_off), 2, 16, _p(q), 2, 3, 1, 10, out=o)
    assert (st, e.value) == (UN, MAX_READ + 1) and o.untouched()
    st, e = _call("bitnuc_reads_edist_adapter_batch_packed", _p(words), _p(woff), None, 10, 16, _p(q), 2, 3, 1, 10, out=o)
    assert st == UN and o.untouched()
    st, e = _call("bitnuc_reads_edist_adapter_batch", _p(s), _p(off), 10, 16, _p(q), 2, 3, 2, 1, out=o)
    assert (st, e.value) == (UN, 2) and o.untouched()
    pats = rp.singletons(q, 16)
    st, e = _call("bitnuc_reads_pattern_edist_adapter", _p(s), 40, 10, 16, C.c_void_p(pats.ctypes.data + 2), 2, 3, 1, 10, out=o)  # patterns: 4-byte aligned
    assert st == UN and o.untouched()


def test_invalid_bytes():
    rng = np.random.default_rng(6)
    k = 16
    q = _random_queries(rng, 3)
    s, off = _reads_with_adapters(rng, [50] * 8, k, q)
    for at in (0, 49, 50, 399, 217):
        t = s.copy()
        t[at] = ord("N")
        t[399] = ord("n") if at != 399 else t[399]
        for pattern in (False, True):
            qq = rp.singletons(q, k) if pattern else q
            st, e, o = _fixed("ascii", t, 50, 8, k, qq, (3, 1, 10), pattern)
            assert (st, e.index, e.byte) == (_status(INVALID_BASE), at, ord("N")) and o.untouched(), at
            st, e, o = _ragged("ascii", t, off, k, qq, (3, 1, 10), pattern)
            assert (st, e.index, e.byte) == (_status(INVALID_BASE), at, ord("N")) and o.untouched(), at
    # a ragged read shorter than k is neither read nor validated: its invalid byte is not reported, it gets the fill
    lens = [40, 7, 40, 15, 0, 16]
    s, off = _reads_with_adapters(rng, lens, k, q)
    want = ao.reads_edist_adapter_batch(s, off, k, q, 3, 1, 10)
    t = s.copy()
    t[int(off[1]) + 3] = ord("N")
    t[int(off[3])] = ord("@")
    st, e, o = _ragged("ascii", t, off, k, q, (3, 1, 10))
    assert st == _status(OK) and _same(o.read(), want)
    t[int(off[5]) + 15] = ord("N")  # the last byte of a read of exactly k bases
    st, e, o = _ragged("ascii", t, off, k, q, (3, 1, 10))
    assert (st, e.index) == (_status(INVALID_BASE), int(off[5]) + 15) and o.untouched()
    # the fixed form validates every read, so a fill-only call (read_len < k) validates nothing
    st, e, o = _fixed("ascii", t, 10, 5, k, q, (3, 1, 10))
    assert st == _status(OK) and _same(o.read(), ao.fill5(5))
