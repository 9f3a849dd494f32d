"""CPU tests of the per-read matchers under pattern queries (bitnuc_reads_pattern_best / _best2 / _best_batch / _anchored / _anchored_batch and their
_packed forms): the host path below the cutoff, through a NULL context, against tests/reads_pattern_oracle.py (itself cross-checked here against the
exact forms' oracles on singleton patterns).  All five families, ASCII and packed; k in {1, 16, 31, 32}; random sets with empty and N positions, IUPAC
strings, singletons against the exact twins byte for byte, junk allow bits at positions >= k, all-N and all-empty patterns, equal patterns, one query;
the argument checks in the exact twins' order with the guarded outputs untouched; the patterns' alignment (4 mod 8 accepted, 2 mod 4 Unsupported); an N
in a read inside and outside the spans; and the five host headers with PatternSets queries under ASan + UBSan in a stand-alone program
(tests/c/reads_pattern_host_sanitize.cpp).  Every comparison is exact equality of all written arrays; guard words and bytes surround the outputs, the
dist arrays start at odd byte offsets; ASCII data carries lowercase bases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pattern_oracle as po
import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_anchored_oracle as ra
import reads_batch_oracle as rb
import reads_anchored_batch_oracle as rab
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
SIZE_MAX = C.c_size_t(-1).value
START, END = 0, 1
FIXED = ("best", "best2", "anchored")
RAGGED = ("best_batch", "anchored_batch")
TRIPLES = {"best": 1, "best2": 2, "anchored": 2, "best_batch": 1, "anchored_batch": 2}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


class Out:
    """up to six outputs inside guarded host buffers: GUARD words around query / pos, the dist arrays at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(4)]
        self.d = [np.full(off + count + GUARD, 0x5A, dtype=np.uint8) for off in (1, 3)]

    def ptrs(self, triples=2, second=True):
        w = [C.c_void_p(a.ctypes.data + 4 * GUARD) for a in self.w]
        d = [C.c_void_p(a.ctypes.data + off) for a, off in zip(self.d, (1, 3))]
        if triples == 1:
            return (w[0], w[1], d[0])
        return (w[0], w[1], d[0], w[2], w[3], d[1]) if second else (w[0], w[1], d[0], None, None, None)

    def untouched(self):
        return all((a == FILL32).all() for a in self.w) and all((a == 0x5A).all() for a in self.d)

    def read(self, triples=2):
        n = self.count
        for a in self.w:
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        six = (w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy())
        return six[:3 * triples]


def _fn(kind, family, packed):
    from bitnuc_amd import _lib as L
    return getattr(L.load(), f"bitnuc_reads_{kind}_{family}" + ("_packed" if packed else ""))


def _queries(kind, queries):
    if kind == "pattern":
        return rp.as_patterns(queries)
    return np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    return fn(*args, C.byref(err)), err


def _fixed(kind, family, packed, s, read_len, count, k, queries, lo=0, hi=None, words=None, qptr=None, nq=None):
    """a fixed-length host entry point with guarded outputs: (status, err, Out)"""
    q = _queries(kind, queries)
    data = (ro.pack_reads(s, read_len, count) if words is None else words) if packed else s
    rng = (lo, SIZE_MAX if hi is None else hi) if family == "anchored" else ()
    o = Out(count)
    st, e = _raw(_fn(kind, family, packed), None, _p(data), read_len, count, k, *rng, _p(q) if qptr is None else qptr, len(q) if nq is None else nq,
                 *o.ptrs(TRIPLES[family]))
    return st, e, o


def _ragged(kind, family, packed, s, off, k, queries, anchor=START, lo=0, hi=0, words=None, qptr=None, nq=None):
    q = _queries(kind, queries)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count = off.size - 1
    woff = rb.word_offsets_of(off)  # (named: the arrays behind the pointers live until the call returns)
    words = (rb.pack_batch(s, off, seed=k) if words is None else words) if packed else None
    head = (_p(words), _p(woff), _p(off)) if packed else (_p(s), _p(off))
    rng = (anchor, lo, hi) if family == "anchored_batch" else ()
    o = Out(count)
    st, e = _raw(_fn(kind, family, packed), None, *head, count, k, *rng, _p(q) if qptr is None else qptr, len(q) if nq is None else nq,
                 *o.ptrs(TRIPLES[family]))
    return st, e, o


def _want_fixed(family, s, read_len, count, k, patterns, lo=0, hi=None):
    if family == "anchored":
        return rp.reads_anchored(s, read_len, count, k, patterns, lo, hi)
    return rp.reads_best2(s, read_len, count, k, patterns)[:3 * TRIPLES[family]]


def _want_ragged(family, s, off, k, patterns, anchor=START, lo=0, hi=0):
    if family == "anchored_batch":
        return rp.reads_anchored_batch(s, off, k, patterns, anchor, lo, hi)
    return rp.reads_best_batch(s, off, k, patterns)


def _random_patterns(rng, nq, k, junk=True):
    """random sets (empty and N positions included); junk: random allow bits at positions >= k (k < 32), which the library must ignore"""
    ps = np.stack([po.from_sets(po.random_sets(rng, k)) for _ in range(nq)])
    if junk and k < 32:
        ps = ps | (rng.integers(0, 2**32, size=ps.shape, dtype=np.uint64) << np.uint64(k)).astype(np.uint32)
    return np.ascontiguousarray(ps.astype(np.uint32))


def _instance(rng, pattern, k):
    """codes of a window that matches the pattern wherever a set is not empty"""
    out = np.zeros(k, dtype=np.int64)
    for i in range(k):
        ok = [c for c in range(4) if (int(pattern[c]) >> i) & 1]
        out[i] = rng.choice(ok) if ok else rng.integers(0, 4)
    return out


def _ascii(rng, codes):
    s = ro.LUT[codes].astype(np.uint8)
    s[rng.random(s.size) < 0.3] |= 0x20
    return s


def _fixed_reads(rng, read_len, count, k, patterns, plant=6):
    codes = rng.integers(0, 4, size=(count, read_len))
    for _ in range(plant if read_len >= k and len(patterns) else 0):
        r, i, q = rng.integers(0, count), rng.integers(0, read_len - k + 1), rng.integers(0, len(patterns))
        codes[r, i:i + k] = _instance(rng, patterns[q], k)
    return _ascii(rng, codes.reshape(-1))


def _ragged_reads(rng, lengths, k, patterns, plant=6):
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    long = [r for r, n in enumerate(lengths) if n >= k]
    for _ in range(plant if long and len(patterns) else 0):
        r, q = long[rng.integers(0, len(long))], rng.integers(0, len(patterns))
        i = int(off[r]) + rng.integers(0, lengths[r] - k + 1)
        codes[i:i + k] = _instance(rng, patterns[q], k)
    return _ascii(rng, codes), off


# ---- the oracle itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_oracle_agrees_with_the_exact_forms_oracles_on_singletons(k):
    rng = np.random.default_rng(900 + k)
    nq, read_len, count = 5, 45, 11
    queries = ro.random_queries(rng, nq, k)
    queries[3] = queries[1]  # an equal query: the runner-up of its twin
    single = rp.singletons(queries, k)
    s = ro.random_reads(rng, read_len, count, k, queries)
    assert _same(rp.reads_best2(s, read_len, count, k, single), r2.reads_best2(s, read_len, count, k, queries))
    assert _same(rp.reads_best2(s, read_len, count, k, single[:1]), r2.reads_best2(s, read_len, count, k, queries[:1]))
    for lo, hi in ((0, 0), (3, 6), (read_len - k - 2, None), (read_len - k + 1, None), (4, 2)):
        assert _same(rp.reads_anchored(s, read_len, count, k, single, lo, hi), ra.reads_anchored(s, read_len, count, k, queries, lo, hi)), (lo, hi)
    lengths = rab.lengths_all_n(k, 2, 4)
    sb, off = rb.random_batch(rng, lengths, k, queries)
    assert _same(rp.reads_best_batch(sb, off, k, single), rb.batch_best(sb, off, k, queries))
    for anchor in (START, END):
        assert _same(rp.reads_anchored_batch(sb, off, k, single, anchor, 2, 5), rab.reads_anchored_batch(sb, off, k, queries, anchor, 2, 5))
    assert _same(rp.reads_best2(s, read_len, count, k, single[:0]), rp.fill6(count)) and _same(rp.reads_best2(s, read_len, count, 0, single), rp.fill6(count))


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_pattern_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads pattern host ok" in out.stdout


# ---- all five families against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_fixed_families_random_sets_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0x9A7 + k)
    for read_len, count in ((k, 3), (k + 7, 9), (70, 13)):
        for nq in (1, 3, 17):
            patterns = _random_patterns(rng, nq, k)
            s = _fixed_reads(rng, read_len, count, k, patterns)
            words = ro.pack_reads(s, read_len, count)
            last = read_len - k
            for family in FIXED:
                ranges = ((0, None),) if family != "anchored" else ((0, 0), (0, min(3, last)), (max(0, last - 3), None), (last // 2, last // 2 + 64 - k))
                for lo, hi in ranges:
                    want = _want_fixed(family, s, read_len, count, k, patterns, lo, hi)
                    for packed in (False, True):
                        st, _, o = _fixed("pattern", family, packed, s, read_len, count, k, patterns, lo, hi, words=words)
                        assert st == L.OK and _same(o.read(TRIPLES[family]), want), (family, packed, k, read_len, nq, lo, hi)


@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_ragged_families_random_sets_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0xBA9 + k)
    for width, lo in ((1, 0), (4, 0), (4, 5), (64 - k + 1, 0)):
        hi = lo + width - 1
        lengths = rab.lengths_all_n(k, lo, width)
        rng.shuffle(lengths)
        for nq in (1, 2, 17):
            patterns = _random_patterns(rng, nq, k)
            s, off = _ragged_reads(rng, lengths, k, patterns)
            words = rb.pack_batch(s, off, seed=width)
            for packed in (False, True):
                st, _, o = _ragged("pattern", "best_batch", packed, s, off, k, patterns, words=words)
                assert st == L.OK and _same(o.read(1), _want_ragged("best_batch", s, off, k, patterns)), (packed, k, nq)
                for anchor in (START, END):
                    want = rp.reads_anchored_batch(s, off, k, patterns, anchor, lo, hi)
                    st, _, o = _ragged("pattern", "anchored_batch", packed, s, off, k, patterns, anchor, lo, hi, words=words)
                    assert st == L.OK and _same(o.read(2), want), (packed, k, nq, anchor, lo, hi)


def test_iupac_strings_through_the_numpy_wrappers():
    """every method of the context-free API, patterns given as IUPAC strings and as a (Q, 4) array: the second triple of the anchored forms optional"""
    free = _free()
    rng = np.random.default_rng(77)
    k = 12
    letters = ["ACGTNNNNACGT", "RYSWKMBDHVNA", "acgtryswkmnn", "NNNNNNNNNNNN", "TTTTTTGGGGGG"]
    patterns = np.stack([po.from_iupac(x) for x in letters])
    read_len, count = 40, 17
    s = _fixed_reads(rng, read_len, count, k, patterns)
    words = ro.pack_reads(s, read_len, count)
    want2 = rp.reads_best2(s, read_len, count, k, patterns)
    for pats in (letters, patterns):
        assert _same(free.reads_pattern_best(s, read_len, k, pats), want2[:3])
        assert _same(free.reads_pattern_best_packed(words, read_len, count, k, pats), want2[:3])
        assert _same(free.reads_pattern_best2(s, read_len, k, pats), want2)
        assert _same(free.reads_pattern_best2_packed(words, read_len, count, k, pats), want2)
        wa = rp.reads_anchored(s, read_len, count, k, patterns, 3, 9)
        assert _same(free.reads_pattern_anchored(s, read_len, k, pats, pos_lo=3, pos_hi=9), wa)
        assert _same(free.reads_pattern_anchored_packed(words, read_len, count, k, pats, pos_lo=3, pos_hi=9, second=False), wa[:3])
    lengths = rab.lengths_all_n(k, 1, 4)
    sb, off = _ragged_reads(rng, lengths, k, patterns)
    wb, woff = rb.pack_batch(sb, off), rb.word_offsets_of(off)
    assert _same(free.reads_pattern_best_batch(sb, off, k, letters), rp.reads_best_batch(sb, off, k, patterns))
    assert _same(free.reads_pattern_best_batch_packed(wb, woff, off, k, letters), rp.reads_best_batch(sb, off, k, patterns))
    for anchor, name in ((START, "start"), (END, "end")):
        want = rp.reads_anchored_batch(sb, off, k, patterns, anchor, 1, 4)
        assert _same(free.reads_pattern_anchored_batch(sb, off, k, letters, pos_lo=1, pos_hi=4, anchor=name), want)
        assert _same(free.reads_pattern_anchored_batch_packed(wb, woff, off, k, patterns, pos_lo=1, pos_hi=4, anchor=name, second=False), want[:3])
    with pytest.raises(ValueError):
        free.reads_pattern_best(s, read_len, k, ["ACGT"])  # four letters for k = 12


@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_singletons_equal_the_exact_twins_byte_for_byte(k):
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0x51 + k)
    queries = ro.random_queries(rng, 9, k)
    queries[6] = queries[2]
    single = rp.singletons(queries, k)
    read_len, count = 66, 21
    s = ro.random_reads(rng, read_len, count, k, queries)
    words = ro.pack_reads(s, read_len, count)
    for family in FIXED:
        for lo, hi in (((0, None),) if family != "anchored" else ((0, 3), (read_len - k - 3, None), (10, 10 + 63 - k))):
            for packed in (False, True):
                a = _fixed("pattern", family, packed, s, read_len, count, k, single, lo, hi, words=words)
                b = _fixed("hdist", family, packed, s, read_len, count, k, queries, lo, hi, words=words)
                assert a[0] == b[0] == L.OK and _same(a[2].read(TRIPLES[family]), b[2].read(TRIPLES[family])), (family, packed, lo, hi)
    lengths = rab.lengths_all_n(k, 2, 4)
    sb, off = rb.random_batch(rng, lengths, k, queries)
    wb = rb.pack_batch(sb, off)
    for family in RAGGED:
        for anchor in (START, END):
            for packed in (False, True):
                a = _ragged("pattern", family, packed, sb, off, k, single, anchor, 2, 5, words=wb)
                b = _ragged("hdist", family, packed, sb, off, k, queries, anchor, 2, 5, words=wb)
                assert a[0] == b[0] == L.OK and _same(a[2].read(TRIPLES[family]), b[2].read(TRIPLES[family])), (family, packed, anchor)


def test_allow_bits_at_positions_above_k_are_ignored():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(0x10)
    for k in (1, 5, 16, 31):
        clean = _random_patterns(rng, 4, k, junk=False)
        junk = clean | np.uint32((0xFFFFFFFF << k) & 0xFFFFFFFF)
        read_len, count = 50, 10
        s = _fixed_reads(rng, read_len, count, k, clean)
        for family in FIXED:
            for packed in (False, True):
                a = _fixed("pattern", family, packed, s, read_len, count, k, junk, 2, 9)
                b = _fixed("pattern", family, packed, s, read_len, count, k, clean, 2, 9)
                assert a[0] == L.OK and _same(a[2].read(TRIPLES[family]), b[2].read(TRIPLES[family]))
                assert _same(a[2].read(TRIPLES[family]), _want_fixed(family, s, read_len, count, k, clean, 2, 9))
        sb, off = _ragged_reads(rng, rab.lengths_all_n(k, 0, 4), k, clean)
        for family in RAGGED:
            for packed in (False, True):
                a = _ragged("pattern", family, packed, sb, off, k, junk, END, 0, 3)
                assert a[0] == L.OK and _same(a[2].read(TRIPLES[family]), _want_ragged(family, sb, off, k, clean, END, 0, 3))


@pytest.mark.parametrize("k", [1, 16, 32])
def test_all_n_all_empty_equal_patterns_and_one_query(k):
    free = _free()
    rng = np.random.default_rng(0xA11 + k)
    read_len, count = k + 9, 7
    ones = np.uint32((1 << k) - 1 if k < 32 else 0xFFFFFFFF)
    all_n, empty = np.full(4, ones, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    other = po.from_sets(po.random_sets(rng, k))
    s = _ascii(rng, rng.integers(0, 4, size=read_len * count))
    words = ro.pack_reads(s, read_len, count)
    zeros, c = np.zeros(count, dtype=np.uint32), count
    # all-N: distance 0 everywhere, so the tie rule decides: query 0 at the lowest offset, the equal pattern at index 2 is the runner-up at the same offset
    for got in (free.reads_pattern_best2(s, read_len, k, [all_n, other, all_n]), free.reads_pattern_best2_packed(words, read_len, c, k, [all_n, other, all_n])):
        d_other = rp.reads_best2(s, read_len, c, k, [other])[2]
        assert _same(got[:3], (zeros, zeros, np.zeros(c, dtype=np.uint8))) and _same(got, rp.reads_best2(s, read_len, c, k, [all_n, other, all_n]))
        assert (got[3] == np.where(d_other == 0, 1, 2)).all() and (got[5] == 0).all()
    got = free.reads_pattern_anchored(s, read_len, k, [other, all_n, all_n], pos_lo=2, pos_hi=5)
    assert _same(got, rp.reads_anchored(s, read_len, c, k, [other, all_n, all_n], 2, 5)) and (got[2] == 0).all() and (got[5] == 0).all()
    assert set(got[0].tolist()) <= {0, 1} and (got[3][got[0] == 1] == 2).all() and (got[4][got[0] == 1] == 2).all()
    # all-empty: distance k everywhere: query 0, offset 0 (or pos_lo); two of them: the second is the runner-up at distance k
    got = free.reads_pattern_best2(s, read_len, k, [empty, empty])
    assert _same(got, (zeros, zeros, np.full(c, k, dtype=np.uint8), zeros + 1, zeros, np.full(c, k, dtype=np.uint8)))
    got = free.reads_pattern_anchored_packed(words, read_len, c, k, [empty, empty], pos_lo=3, pos_hi=4)
    assert _same(got, (zeros, zeros + 3, np.full(c, k, dtype=np.uint8), zeros + 1, zeros + 3, np.full(c, k, dtype=np.uint8)))
    # one query: the fill in the second triple
    for got in (free.reads_pattern_best2(s, read_len, k, [other]), free.reads_pattern_anchored(s, read_len, k, [other], pos_lo=0, pos_hi=4)):
        assert _same(got[3:], rp.fill6(c)[3:]) and (got[2] <= k).all()
    # ragged: the same rules per read; reads without a window get the fill in all six
    lengths = [0, k - 1, k, k + 3, 90] if k > 1 else [0, 1, 4, 90]
    sb, off = _ragged_reads(rng, lengths, k, [other])
    for anchor in ("start", "end"):
        got = free.reads_pattern_anchored_batch(sb, off, k, [all_n, all_n], pos_lo=0, pos_hi=3, anchor=anchor)
        assert _same(got, rp.reads_anchored_batch(sb, off, k, [all_n, all_n], anchor, 0, 3))
        has = np.diff(off.astype(np.int64)) >= k
        assert (got[2][has] == 0).all() and (got[0][has] == 0).all() and (got[3][has] == 1).all() and (got[2][~has] == 0xFF).all() and (got[3][~has] == rp.NO_U32).all()
    got = free.reads_pattern_best_batch(sb, off, k, [empty, all_n])
    assert (got[0][has] == 1).all() and (got[1][has] == 0).all() and (got[2][has] == 0).all() and (got[0][~has] == rp.NO_U32).all()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_follow_the_exact_twins_in_order_with_outputs_untouched():
    """Every failing call of the exact twins' own check lists, made on both kinds with the same arguments (the queries' pointer apart): the same status,
    value and index, and nothing written.  Then what differs: the patterns' alignment."""
    from bitnuc_amd import _lib as L
    k, read_len, count = 5, 20, 4
    s = np.frombuffer(b"ACGTACGTAC" * 8, dtype=np.uint8).copy()
    words = ro.pack_reads(s, read_len, count)
    off = rb.offsets_of([read_len] * count)
    q64 = np.zeros(8, dtype=np.uint64)
    pat = np.zeros((8, 4), dtype=np.uint32)
    NULL = C.c_void_p(None)
    decreasing = np.array([0, 9, 3, 3, 3], dtype=np.uint64)

    def both(family, packed, ragged, **kw):
        res = []
        for kind, arr in (("hdist", q64), ("pattern", pat)):
            a = dict(kw)
            if a.get("qptr") == "null":
                a["qptr"] = NULL
            elif "qptr" not in a:
                a["qptr"] = _p(arr)
            if ragged:
                st, e, o = _ragged(kind, family, packed, a.pop("s", s), a.pop("off", off), a.pop("k", k), arr[:2], END, a.pop("lo", 0), a.pop("hi", 3), words=words, **a)
            else:
                st, e, o = _fixed(kind, family, packed, a.pop("s", s), read_len, a.pop("count", count), a.pop("k", k), arr[:2], a.pop("lo", 0), a.pop("hi", 3),
                                  words=words, **a)
            res.append((st, e.value, e.index, o.untouched()))
        assert res[0] == res[1], (family, packed, kw, res)
        return res[1]

    for family in FIXED + RAGGED:
        ragged = family in RAGGED
        for packed in (False, True):
            assert both(family, packed, ragged, k=33, nq=70000, qptr="null")[:2] == (L.SEQUENCE_TOO_LONG, 33)       # k before the query limit
            assert both(family, packed, ragged, nq=65537, qptr="null")[:2] == (L.UNSUPPORTED, 65537)                   # the limit before the arrays
            assert both(family, packed, ragged, qptr="null", nq=2)[0] == L.UNSUPPORTED                                 # queries NULL with n_queries > 0
            if family == "anchored_batch":
                assert both(family, packed, True, lo=0, hi=70, qptr="null", nq=2)[:2] == (L.UNSUPPORTED, 71 + k - 1)  # the span before the arrays
            if ragged:
                assert both(family, packed, True, off=decreasing)[0] == L.INVALID_RANGE                                # the tables' faults
        # count == 0: OK and nothing written, even with NULL queries
        if not ragged:
            assert both(family, False, False, count=0, qptr="null", nq=3) == (L.OK, 0, 0, True)
    # an output NULL or misaligned, on both kinds (the best family stands for the shared check)
    for kind, arr in (("hdist", q64), ("pattern", pat)):
        for bad in range(3):
            o = Out(count)
            ptrs = list(o.ptrs(1))
            ptrs[bad] = None
            st, e = _raw(_fn(kind, "best", False), None, _p(s), read_len, count, k, _p(arr), 2, *ptrs)
            assert st == L.UNSUPPORTED and o.untouched()
        o = Out(count)
        ptrs = list(o.ptrs(1))
        ptrs[1] = C.c_void_p(ptrs[1].value + 2)
        st, e = _raw(_fn(kind, "best", False), None, _p(s), read_len, count, k, _p(arr), 2, *ptrs)
        assert st == L.UNSUPPORTED and o.untouched()
    # the _async forms check the context first
    lib = L.load()
    st, e = _raw(lib.bitnuc_reads_pattern_best_async, None, None, 2**40, 2**40, 40, None, 70000, None, None, None)
    assert st == L.UNSUPPORTED and e.value == 0
    st, e = _raw(lib.bitnuc_reads_pattern_anchored_batch_packed_async, None, None, None, None, 2**40, 2**60, 40, 7, 0, SIZE_MAX, None, 70000, *([None] * 6))
    assert st == L.UNSUPPORTED and e.value == 0


def test_a_pattern_pointer_at_4_mod_8_is_accepted_and_at_2_mod_4_is_unsupported():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(48)
    k, read_len, count = 9, 30, 6
    patterns = _random_patterns(rng, 3, k)
    s = _fixed_reads(rng, read_len, count, k, patterns)
    off = rb.offsets_of([read_len] * count)
    buf = np.zeros(3 * 4 + 4, dtype=np.uint32)
    base = buf.ctypes.data
    at = 1 if (base + 4) % 8 == 4 else 2  # the dword at 4 mod 8
    assert (base + 4 * at) % 8 == 4
    buf[at:at + 12] = patterns.reshape(-1)
    shifted = C.c_void_p(base + 4 * at)
    odd = C.c_void_p(base + 4 * at + 2)
    for family in FIXED:
        for packed in (False, True):
            st, _, o = _fixed("pattern", family, packed, s, read_len, count, k, patterns, 1, 6, qptr=shifted)
            assert st == L.OK and _same(o.read(TRIPLES[family]), _want_fixed(family, s, read_len, count, k, patterns, 1, 6)), (family, packed)
            st, e, o = _fixed("pattern", family, packed, s, read_len, count, k, patterns, 1, 6, qptr=odd)
            assert st == L.UNSUPPORTED and o.untouched(), (family, packed)
    for family in RAGGED:
        for packed in (False, True):
            st, _, o = _ragged("pattern", family, packed, s, off, k, patterns, START, 1, 6, qptr=shifted)
            assert st == L.OK and _same(o.read(TRIPLES[family]), _want_ragged(family, s, off, k, patterns, START, 1, 6)), (family, packed)
            st, e, o = _ragged("pattern", family, packed, s, off, k, patterns, START, 1, 6, qptr=odd)
            assert st == L.UNSUPPORTED and o.untouched(), (family, packed)


def test_an_n_in_a_read_is_still_an_invalid_base_inside_the_spans_and_ignored_outside():
    """the sets are on the query's side: an all-N pattern does not make an N in a read valid"""
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(5)
    k, read_len, count = 8, 40, 5
    ones = np.uint32(0xFF)
    patterns = np.stack([np.full(4, ones, dtype=np.uint32), po.from_iupac("ACGTNNRY")])
    s = _fixed_reads(rng, read_len, count, k, patterns)
    off = rb.offsets_of([read_len] * count)
    bad = s.copy()
    at = 2 * read_len + 30  # read 2, base 30: inside every whole-read scan, outside the anchored range 2 .. 5 (bases 2 .. 12)
    bad[at] = ord("N")
    for family in ("best", "best2"):
        st, e, o = _fixed("pattern", family, False, bad, read_len, count, k, patterns)
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), at) and o.untouched()
    st, e, o = _ragged("pattern", "best_batch", False, bad, off, k, patterns)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), at) and o.untouched()
    st, e, o = _fixed("pattern", "anchored", False, bad, read_len, count, k, patterns, 2, 5)
    assert st == L.OK and _same(o.read(2), rp.reads_anchored(s, read_len, count, k, patterns, 2, 5))
    st, e, o = _ragged("pattern", "anchored_batch", False, bad, off, k, patterns, START, 2, 5)
    assert st == L.OK and _same(o.read(2), rp.reads_anchored_batch(s, off, k, patterns, START, 2, 5))
    bad[2 * read_len + 12] = ord("n")  # the last base of the span
    st, e, o = _fixed("pattern", "anchored", False, bad, read_len, count, k, patterns, 2, 5)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("n"), 2 * read_len + 12) and o.untouched()
    st, e, o = _ragged("pattern", "anchored_batch", False, bad, off, k, patterns, START, 2, 5)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("n"), 2 * read_len + 12) and o.untouched()


def test_host_cutoff_is_judged_as_the_exact_twins_judge_it():
    """below the cutoff (2^20 windows x queries) no context is needed; above it a NULL context is Unsupported and nothing is written"""
    from bitnuc_amd import _lib as L
    count, k, read_len = 23625, 16, 19  # four windows per read: 94,500 in all; x 11 < 2^20 <= x 12
    rng = np.random.default_rng(1)
    s = _ascii(rng, rng.integers(0, 4, size=count * read_len))
    off = rb.offsets_of([read_len] * count)
    words, wb = ro.pack_reads(s, read_len, count), rb.pack_batch(s, off)
    for nq, host in ((11, True), (12, False)):
        patterns = _random_patterns(rng, nq, k)
        for packed in (False, True):
            for family in FIXED:
                st, _, o = _fixed("pattern", family, packed, s, read_len, count, k, patterns, 0, 3, words=words)
                assert st == (L.OK if host else L.UNSUPPORTED) and (host or o.untouched()), (family, nq)
            for family in RAGGED:
                st, _, o = _ragged("pattern", family, packed, s, off, k, patterns, START, 0, 3, words=wb)
                assert st == (L.OK if host else L.UNSUPPORTED) and (host or o.untouched()), (family, nq)
