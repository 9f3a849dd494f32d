"""CPU tests of the anchored best match and runner-up per read of a RAGGED batch (bitnuc_reads_hdist_anchored_batch / _batch_packed): the host path below
the cutoff, through a NULL context, against tests/reads_anchored_batch_oracle.py -- k in {1, 2, 16, 31, 32}; both anchors; ranges of 1, 2, 4 and
64 - k + 1 offsets at pos_lo 0 and > 0; length mixes with 0, 1 .. k - 1, exactly k, exactly enough for all offsets and one base fewer, and much longer;
the ten argument checks in order with the guarded outputs untouched; span 64 accepted, span 65 and pos_hi = SIZE_MAX Unsupported with their value; the
table faults as reads_hdist_best_batch reports them; the second triple all NULL or partly NULL; an N inside a span reported with its absolute index, an N
behind a span, in the bases behind an END range with pos_lo > 0 or anywhere in a read without a window ignored; the cutoff judged on count x offsets x
queries; the identities with reads_hdist_anchored (START and END on equal lengths) and reads_hdist_best_batch (reads <= 64, START (0, 64 - k)); and the
host helpers (csrc/reads_anchored_batch_host.h) under ASan + UBSan in a stand-alone program (tests/c/reads_anchored_batch_host_sanitize.cpp).
Every comparison is exact equality of all written arrays; guard words and bytes surround the six outputs, both dist arrays start at odd byte offsets;
ASCII data carries lowercase bases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_best_oracle as ro
import reads_best2_oracle as r2
import reads_batch_oracle as rb
import reads_anchored_batch_oracle as rab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
SIZE_MAX = C.c_size_t(-1).value
START, END = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _raw(fn, *args):
    from bitnuc_amd import _lib as L
    err = L.BitnucErr()
    st = fn(*args, C.byref(err))
    return st, err


class Out:
    """the six outputs inside guarded host buffers: GUARD words around query / pos, the dist arrays at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(4)]  # best_query, best_pos, second_query, second_pos
        self.d = [np.full(off + count + GUARD, 0x5A, dtype=np.uint8) for off in (1, 3)]

    def ptrs(self, second=True):
        w = [C.c_void_p(a.ctypes.data + 4 * GUARD) for a in self.w]
        d = [C.c_void_p(a.ctypes.data + off) for a, off in zip(self.d, (1, 3))]
        return (w[0], w[1], d[0], w[2], w[3], d[1]) if second else (w[0], w[1], d[0], None, None, None)

    def untouched(self, which=(0, 1)):
        return all((self.w[2 * j + i] == FILL32).all() for j in which for i in (0, 1)) and all((self.d[j] == 0x5A).all() for j in which)

    def read(self):
        n = self.count
        for a in self.w:
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / pos written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        return w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy()


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, second=True, words=None, woff=None):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count = off.size - 1
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    o = Out(count)
    if form == "ascii":
        st, e = _raw(lib.bitnuc_reads_hdist_anchored_batch, None, _p(s), _p(off), count, k, anchor, pos_lo, pos_hi, _p(q), q.size, *o.ptrs(second))
    else:
        woff = rb.word_offsets_of(off) if woff is None else woff
        words = rb.pack_batch(s, off, seed=k) if words is None else words
        st, e = _raw(lib.bitnuc_reads_hdist_anchored_batch_packed, None, _p(words), _p(woff), _p(off), count, k, anchor, pos_lo, pos_hi, _p(q), q.size, *o.ptrs(second))
    return st, e, o


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_anchored_batch_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads anchored batch host ok" in out.stdout


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_host_path_grid_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0xBA7C + k)
    for width in (1, 2, 4, 64 - k + 1):
        for pos_lo in (0, 5):
            pos_hi = pos_lo + width - 1
            lengths = rab.lengths_all_n(k, pos_lo, width)
            rng.shuffle(lengths)
            for nq in (1, 2, 17):
                queries = ro.random_queries(rng, nq, k)
                s, off = rb.random_batch(rng, lengths, k, queries)
                woff, words = rb.word_offsets_of(off), rb.pack_batch(s, off, seed=width)
                for anchor in (START, END):
                    want = rab.reads_anchored_batch(s, off, k, queries, anchor, pos_lo, pos_hi)
                    first, n = rab.windows(np.diff(off.astype(np.int64)), k, anchor, pos_lo, pos_hi)
                    assert set(range(width + 1)) <= set(n.tolist())  # every number of admissible offsets, 0 included
                    assert ((want[2] == 0xFF) == (n == 0)).all() and (want[1][n > 0] >= first[n > 0]).all() and (want[1][n > 0] < (first + n)[n > 0]).all()
                    for form in ("ascii", "packed"):
                        st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, words=words, woff=woff)
                        assert st == L.OK and _same(o.read(), want), (form, k, width, pos_lo, nq, anchor)
                        st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, second=False, words=words, woff=woff)  # the best triple only
                        assert st == L.OK and _same(o.read()[:3], want[:3]) and o.untouched(which=(1,)), (form, k, width, pos_lo, nq, anchor)
            got = free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end")  # the numpy wrappers
            assert _same(got, want)
            assert _same(free.reads_hdist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end"), want)
            assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor=1, second=False), want[:3])


def test_end_anchor_follows_each_reads_own_end():
    """END, 0, 0 is the last k bases; END, 0, 3 the last k bases with three bases of slack; END, 2, 3 leaves the last two bases out"""
    free = _free()
    k = 6
    q = ro.word_of([0, 1, 2, 3, 0, 1])  # ACGTAC
    reads = [b"TTTTTTTTACGTAC", b"GGACGTAC", b"ACGTAC", b"ACGTA", b"", b"ggggACGTACtt", b"ACGTACggg", b"ACGTACgggg"]
    s = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    off = rb.offsets_of([len(r) for r in reads])
    got = free.reads_hdist_anchored_batch(s, off, k, [q], pos_lo=0, pos_hi=0, anchor="end")
    assert got[1].tolist()[:4] == [8, 2, 0, ro.NO_U32] and got[2].tolist()[:5] == [0, 0, 0, 0xFF, 0xFF] and got[2][5] > 0
    got = free.reads_hdist_anchored_batch(s, off, k, [q], pos_lo=0, pos_hi=3, anchor="end")
    assert got[2].tolist() == [0, 0, 0, 0xFF, 0xFF, 0, 0, got[2][7]] and got[2][7] > 0 and got[1].tolist()[5:7] == [4, 0]
    got = free.reads_hdist_anchored_batch(s, off, k, [q], pos_lo=2, pos_hi=3, anchor="end")
    assert got[2][5] == 0 and got[2][6] == 0 and got[2][0] > 0 and (got[3] == ro.NO_U32).all()  # one query: no runner-up
    for lo, hi in ((0, 0), (0, 3), (2, 3)):
        assert _same(free.reads_hdist_anchored_batch(s, off, k, [q], pos_lo=lo, pos_hi=hi, anchor="end"), rab.reads_anchored_batch(s, off, k, [q], END, lo, hi))


def test_ties_duplicates_and_the_winners_second_window():
    free = _free()
    rng = np.random.default_rng(35)
    k, nq = 20, 24
    queries = ro.random_queries(rng, nq, k)
    queries[20] = queries[3] ^ (np.uint64(1) << np.uint64(63))  # an equal duplicate of query 3 at index 20 (junk above 2k differs)
    lengths = [90, 61, 75, 50, 66, 20, 19]
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    q3, q5, q12 = (ro.query_codes(queries[i], k) for i in (3, 5, 12))
    near5 = q5.copy()
    near5[[2, 9]] ^= 1
    o = [int(x) for x in off]
    # END (2, 12): read 0 (last 70) admits 58 .. 68, read 1 (last 41) 29 .. 39, read 2 (last 55) 43 .. 53, read 3 (last 30) 18 .. 28, read 4 (last 46) 34 .. 44
    codes[o[0] + 60:o[0] + 60 + k] = q3                                         # read 0: query 3 and its duplicate exactly
    codes[o[1] + 28:o[1] + 28 + k], codes[o[1] + 5:o[1] + 5 + k] = q5, near5   # read 1: an exact copy one base in front of the range, none inside
    codes[o[2] + 54:o[2] + 54 + k], codes[o[2] + 20:o[2] + 20 + k] = q5, near5 # read 2: an exact copy one base behind the range
    codes[o[3] + 28:o[3] + 28 + k] = q12                                        # read 3: a match at the last admissible offset
    codes[o[4] + 34:o[4] + 34 + k] = q12                                        # read 4: at the first
    s = ro.LUT[codes].astype(np.uint8)
    s[::3] |= 0x20
    want = rab.reads_anchored_batch(s, off, k, queries, END, 2, 12)
    assert tuple(int(a[0]) for a in want) == (3, 60, 0, 20, 60, 0)
    assert int(want[2][1]) > 0 and int(want[2][2]) > 0 and tuple(int(a[3]) for a in want[:3]) == (12, 28, 0) and int(want[3][3]) != 12
    assert tuple(int(a[4]) for a in want[:3]) == (12, 34, 0) and int(want[3][4]) != 12
    assert int(want[2][5]) == 0xFF and int(want[2][6]) == 0xFF  # 20 bases: last 0 < pos_lo 2; 19 bases: shorter than k
    words, woff = rb.pack_batch(s, off), rb.word_offsets_of(off)
    assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=2, pos_hi=12, anchor="end"), want)
    assert _same(free.reads_hdist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=2, pos_hi=12, anchor="end"), want)
    whole = free.reads_hdist_best_batch(s, off, k, queries)  # the whole-read search finds the copies outside
    assert (int(whole[1][1]), int(whole[2][1])) == (28, 0) and (int(whole[1][2]), int(whole[2][2])) == (54, 0)
    # poly-A reads, a poly-A query at two indices: the lowest query, the lowest offset; the runner-up is the duplicate at the same offset
    qs = np.array([7, 0, 0], dtype=np.uint64)
    s = np.full(int(off[-1]), ord("a"), dtype=np.uint8)
    for anchor, lo, hi in ((START, 3, 9), (END, 3, 9)):
        got = free.reads_hdist_anchored_batch(s, off, k, qs, pos_lo=lo, pos_hi=hi, anchor=anchor)
        assert _same(got, rab.reads_anchored_batch(s, off, k, qs, anchor, lo, hi))
        first, n = rab.windows(lengths, k, anchor, lo, hi)
        assert got[0][n > 0].tolist() == [1] * int((n > 0).sum()) and got[3][n > 0].tolist() == [2] * int((n > 0).sum())
        assert np.array_equal(got[1][n > 0], first[n > 0]) and np.array_equal(got[4][n > 0], first[n > 0])


def test_fills_empty_ranges_no_query_and_count_zero():
    from bitnuc_amd import _lib as L
    lengths = [6, 0, 9]
    s = np.frombuffer(b"ACGTAC" + b"ACGTACGTA", dtype=np.uint8).copy()
    off = rb.offsets_of(lengths)
    for k, queries, pos_lo, pos_hi in ((0, [1, 2], 0, 3), (10, [1, 2], 0, 3), (3, [], 0, 3), (3, [1, 2], 7, 9), (3, [1, 2], 2, 1), (3, [1, 2], SIZE_MAX, SIZE_MAX),
                                       (3, [1, 2], SIZE_MAX - 5, SIZE_MAX), (3, [1, 2], 2**32, 2**32 + 3), (3, [1, 2], 13, 20)):
        for anchor in (START, END):
            for form in ("ascii", "packed"):
                st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi)
                assert st == L.OK and _same(o.read(), r2.fill6(3)), (k, queries, pos_lo, pos_hi)
                st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, second=False)
                assert st == L.OK and _same(o.read()[:3], r2.fill6(3)[:3]) and o.untouched(which=(1,))
            assert _same(rab.reads_anchored_batch(s, off, k, queries, anchor, pos_lo, pos_hi), r2.fill6(3))
    lib = L.load()
    for fn, head in ((lib.bitnuc_reads_hdist_anchored_batch, (_p(s), _p(off))), (lib.bitnuc_reads_hdist_anchored_batch_packed, (_p(s), _p(off), _p(off)))):
        o = Out(3)
        st, _ = _raw(fn, None, *head, 0, 3, START, 0, 3, None, 2, *o.ptrs())  # count == 0: nothing written
        assert st == L.OK and o.untouched()


def test_span_64_is_accepted_65_and_size_max_are_unsupported_with_their_value():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(64)
    lengths = [150, 64, 63, 0, 70, 200]
    for k in (1, 16, 32):
        queries = ro.random_queries(rng, 3, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        for anchor in (START, END):
            for pos_lo in (0, 37, SIZE_MAX - 64):
                for form in ("ascii", "packed"):
                    if pos_lo < 100:
                        want = rab.reads_anchored_batch(s, off, k, queries, anchor, pos_lo, pos_lo + 64 - k)
                        st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_lo + 64 - k)
                        assert st == L.OK and _same(o.read(), want)
                    st, e, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_lo + 65 - k)
                    assert st == L.UNSUPPORTED and e.value == 65 and o.untouched()
            for form in ("ascii", "packed"):
                st, e, o = _call(form, s, off, k, queries, anchor, 0, SIZE_MAX)  # not "to the end of the read": offsets and span do not fit
                assert st == L.UNSUPPORTED and e.value == SIZE_MAX and o.untouched()
                st, e, o = _call(form, s, off, k, queries, anchor, 10, SIZE_MAX)
                assert st == L.UNSUPPORTED and e.value == (SIZE_MAX - 10 + k if k < 11 else SIZE_MAX) and o.untouched()
                st, e, o = _call(form, s, off, k, [], anchor, 0, 200)  # the span is judged on the arguments alone: also without queries
                assert st == L.UNSUPPORTED and e.value == 200 + k and o.untouched()
                st, e, o = _call(form, s, off, k, [], anchor, 0, 64 - k)  # a span of 64 without queries: the fill
                assert st == L.OK and _same(o.read(), r2.fill6(len(lengths)))


def test_table_faults_are_reported_as_best_batch_reports_them():
    from bitnuc_amd import _lib as L
    lib = L.load()
    q = np.zeros(2, dtype=np.uint64)
    s = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    words = np.zeros(16, dtype=np.uint64)
    good = rb.offsets_of([10, 0, 40, 33])
    gw = rb.word_offsets_of(good)
    cases = []
    for name, off, woff in (("decreasing", np.array([0, 10, 9, 50, 83], dtype=np.uint64), gw), ("not from zero", good + np.uint64(1), gw),
                            ("word table", good, gw + np.array([0, 0, 1, 1, 1], dtype=np.uint64)), ("word table from", good, gw + np.uint64(1)),
                            ("long read", np.array([0, 10, 10, 2**32 + 9, 2**32 + 42], dtype=np.uint64), None),
                            ("long batch", np.array([0, 2**32 - 2, 2 * (2**32 - 2), 2**58, 2**58 + 1], dtype=np.uint64), None)):
        cases.append((name, off, woff))
    for name, off, woff in cases:
        for packed in (False, True):
            if woff is None and packed:
                woff = rb.word_offsets_of(off)
            if name.startswith("word table") and not packed:
                continue
            o, o3 = Out(4), Out(4)
            if packed:
                got = _raw(lib.bitnuc_reads_hdist_anchored_batch_packed, None, _p(words), _p(woff), _p(off), 4, 5, END, 0, 3, _p(q), 2, *o.ptrs())
                ref = _raw(lib.bitnuc_reads_hdist_best_batch_packed, None, _p(words), _p(woff), _p(off), 4, 5, _p(q), 2, *o3.ptrs()[:3])
            else:
                got = _raw(lib.bitnuc_reads_hdist_anchored_batch, None, _p(s), _p(off), 4, 5, END, 0, 3, _p(q), 2, *o.ptrs())
                ref = _raw(lib.bitnuc_reads_hdist_best_batch, None, _p(s), _p(off), 4, 5, _p(q), 2, *o3.ptrs()[:3])
            assert got[0] == ref[0] and got[0] in (L.INVALID_RANGE, L.UNSUPPORTED), (name, packed, got[0], ref[0])
            assert (got[1].value, got[1].index) == (ref[1].value, ref[1].index), (name, packed)
            assert o.untouched()


def test_invalid_bytes_inside_a_span_absolute_index_outside_ignored():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(12)
    k, lo, hi = 7, 2, 5
    lengths = [50, 8, 30, 0, 6, 9, 41, 12, 10]
    queries = ro.random_queries(rng, 3, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    o = [int(x) for x in off]
    for anchor in (START, END):
        clean = rab.reads_anchored_batch(s, off, k, queries, anchor, lo, hi)
        mask = rab.span_bytes(off, k, anchor, lo, hi)
        b = s.copy()
        b[~mask] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=int((~mask).sum()))  # every byte no span holds: behind and in front
        # of the spans, the bases behind an END range (pos_lo > 0), every byte of the reads without a window (8 and 6 bases)
        assert not mask[o[1]:o[2]].any() and not mask[o[4]:o[5]].any()
        if anchor == END:
            assert not mask[o[0] + 48] and not mask[o[0] + 49] and mask[o[0] + 47]  # the two bases behind the range of read 0
        st, _, out = _call("ascii", b, off, k, queries, anchor, lo, hi)
        assert st == L.OK and _same(out.read(), clean)
        assert _same(free.reads_hdist_anchored_batch(b, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor), clean)
        spans = np.nonzero(mask)[0]
        later, bad_at = int(spans[-1]), int(spans[np.searchsorted(spans, o[6])])  # read 6's first span byte; a later one in the last read
        b[later] = ord("x")
        b[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            free.reads_hdist_anchored_batch(b, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        st, e, out = _call("ascii", b, off, k, queries, anchor, lo, hi)
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), bad_at) and out.untouched()
        b[bad_at] = s[bad_at]
        st, e, out = _call("ascii", b, off, k, queries, anchor, lo, hi)  # the last span byte of the batch
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("x"), later) and out.untouched()
        st, _, out = _call("ascii", b, off, k, queries, anchor, 60, 70)  # no window: nothing is read or validated
        assert st == L.OK and _same(out.read(), r2.fill6(len(lengths)))


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    best, packed = lib.bitnuc_reads_hdist_anchored_batch, lib.bitnuc_reads_hdist_anchored_batch_packed
    adev, pdev = lib.bitnuc_reads_hdist_anchored_batch_async, lib.bitnuc_reads_hdist_anchored_batch_packed_async
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = _p(s)
    words = np.zeros(9, dtype=np.uint64)
    wp = _p(words)
    off = rb.offsets_of([64, 64, 64, 64])
    woff = rb.word_offsets_of(off)
    short = rb.offsets_of([1, 0, 1, 1])  # three bases in all: no window of five
    q = np.zeros(8, dtype=np.uint64)
    qp = _p(q)
    o = Out(8)
    outs = o.ptrs()
    none6 = (None,) * 6
    bad_tab = C.c_void_p(off.ctypes.data + 4)

    def host(fn, src, tabs, count, k, anchor, lo, hi, qq, nq, six):
        return _raw(fn, None, src, *tabs, count, k, anchor, lo, hi, qq, nq, *six)
    forms = ((best, sp, (_p(off),)), (packed, wp, (_p(woff), _p(off))))
    # 1. the _async forms check the context first, whatever else is wrong
    st, e = _raw(adev, None, None, None, 2**40, 2**60, 40, 7, 0, SIZE_MAX, None, 70000, *none6)
    assert st == L.UNSUPPORTED and e.value == 0
    st, e = _raw(pdev, None, None, None, None, 2**40, 2**60, 40, 7, 0, SIZE_MAX, None, 70000, *none6)
    assert st == L.UNSUPPORTED and e.value == 0
    # 2. k > 32, even with too many queries, a bad anchor, too wide a span and NULL pointers everywhere
    for fn, src, tabs in forms:
        st, e = host(fn, None, (None,) * len(tabs), 2**40, 33, 7, 0, SIZE_MAX, None, 70000, none6)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
    # (3. the totals' limit belongs to the _async forms: the GPU tests; the host forms bound their tables' totals in check 8)
    # 4. too many queries -> Unsupported with the count, before the anchor, the span, count == 0 and the array checks
    for fn, src, tabs in forms:
        st, e = host(fn, None, (None,) * len(tabs), 0, 5, 7, 0, SIZE_MAX, None, 65537, none6)
        assert st == L.UNSUPPORTED and e.value == 65537
    # 5. the anchor (value = anchor), then the span (value = span), before count == 0 and the array checks
    for fn, src, tabs in forms:
        st, e = host(fn, None, (None,) * len(tabs), 0, 5, 2, 10, 80, None, 3, none6)
        assert st == L.UNSUPPORTED and e.value == 2
        st, e = host(fn, None, (None,) * len(tabs), 0, 5, END, 10, 80, None, 3, none6)
        assert st == L.UNSUPPORTED and e.value == 75
    # 6. count == 0: OK, nothing written, even with NULL arrays and tables
    for fn, src, tabs in forms:
        st, e = host(fn, None, (None,) * len(tabs), 0, 5, END, 0, 3, None, 3, none6)
        assert st == L.OK
    # 7. a best output NULL, one or two of the second outputs NULL, a query / pos array of either triple misaligned, queries NULL (with queries) or
    # misaligned, a table NULL or not 8-byte aligned -> Unsupported, before the tables are read (they are invalid: check 8) and the no-window case
    def shifted(i, by):
        return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
    bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
    bad += [(qp, tuple(None if j in pair else p for j, p in enumerate(outs))) for pair in ((3, 4), (3, 5), (4, 5), (0, 3, 4, 5))]
    bad += [(None, outs), (C.c_void_p(q.ctypes.data + 4), outs)]
    bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1)), (qp, shifted(4, 2))]  # (4: second_pos)
    decreasing = np.array([0, 9, 3, 3, 3], dtype=np.uint64)
    for qq, six in bad:
        for fn, src, tabs in ((best, sp, (_p(decreasing),)), (packed, wp, (_p(decreasing), _p(decreasing)))):
            st, e = host(fn, src, tabs, 4, 5, START, 0, 3, qq, 2, six)
            assert st == L.UNSUPPORTED and e.value == 0
    for fn, src, tabs in ((best, sp, (None,)), (best, sp, (bad_tab,)), (packed, wp, (None, _p(off))), (packed, wp, (_p(woff), None)), (packed, wp, (bad_tab, _p(off))),
                          (packed, wp, (_p(woff), bad_tab))):
        st, e = host(fn, src, tabs, 4, 5, START, 0, 3, qp, 2, outs)
        assert st == L.UNSUPPORTED and e.value == 0
    assert o.untouched()
    # 8. the tables' faults, before the no-window case and the NULL data (test_table_faults_... compares them with best_batch's)
    for fn, src, tabs in ((best, None, (_p(decreasing),)), (packed, None, (_p(decreasing), _p(decreasing)))):
        st, e = host(fn, src, tabs, 4, 0, START, 0, 3, qp, 0, outs)
        assert st == L.INVALID_RANGE and e.value == 2
    assert o.untouched()
    # 9. no windows: the fill in [0, count) of all six and nothing after, before the data is looked at (NULL); both dist arrays at odd addresses
    for k, tab, nq, qq, lo, hi in ((0, off, 8, qp, 0, 3), (5, short, 8, qp, 0, 3), (5, off, 0, None, 0, 3), (5, off, 8, qp, 4, 3), (5, off, 8, qp, 252, 260)):
        for fn, tabs in ((best, (_p(tab),)), (packed, (_p(rb.word_offsets_of(tab)), _p(tab)))):
            for anchor in (START, END):
                o = Out(4)
                st, _ = host(fn, None, tabs, 4, k, anchor, lo, hi, qq, nq, o.ptrs())
                assert st == L.OK and _same(o.read(), r2.fill6(4)), (k, nq, lo, hi)
    # 10. then NULL data, or packed words not 8-byte aligned
    o = Out(4)
    outs = o.ptrs()
    st, _ = host(best, None, (_p(off),), 4, 5, START, 0, 3, qp, 8, outs)
    assert st == L.UNSUPPORTED
    st, _ = host(packed, None, (_p(woff), _p(off)), 4, 5, START, 0, 3, qp, 8, outs)
    assert st == L.UNSUPPORTED
    st, _ = host(packed, C.c_void_p(words.ctypes.data + 4), (_p(woff), _p(off)), 4, 5, START, 0, 3, qp, 8, outs)
    assert st == L.UNSUPPORTED
    assert o.untouched()
    # and a valid call writes [0, count) of each output only: AAAAA (queries 0 .. 2, equal) against ACGTACGT...: a window at an offset of 0 mod 4 (ACGTA)
    # differs in 3 bases, every other in 4.  START 1 .. 3: all 4, the lowest offset; END 1 .. 3 (last 59): offsets 56 .. 58, 56 differs in 3
    o = Out(4)
    st, _ = host(best, sp, (_p(off),), 4, 5, START, 1, 3, qp, 3, o.ptrs())
    assert st == L.OK and [list(a) for a in o.read()] == [[0] * 4, [1] * 4, [4] * 4, [1] * 4, [1] * 4, [4] * 4]
    o = Out(4)
    st, _ = host(best, sp, (_p(off),), 4, 5, END, 1, 3, qp, 3, o.ptrs())
    assert st == L.OK and [list(a) for a in o.read()] == [[0] * 4, [56] * 4, [3] * 4, [1] * 4, [56] * 4, [3] * 4]


def test_host_cutoff_is_judged_on_count_times_offsets_times_queries():
    """Below the cutoff (1 Mi offsets x queries) the host forms need no context; above it they do (a NULL context -> Unsupported).  The range's four
    offsets count for every read, whatever its length."""
    from bitnuc_amd import _lib as L
    count, k = 23625, 16  # four offsets per read: 94,500 in all; x 11 < 2^20 <= x 12
    rng = np.random.default_rng(1)
    lengths = rng.integers(0, 60, size=count)
    off = rb.offsets_of(lengths)
    s = ro.LUT[rng.integers(0, 4, size=int(off[-1]))].astype(np.uint8)
    woff, words = rb.word_offsets_of(off), rb.pack_batch(s, off)
    for nq, host in ((11, True), (12, False)):
        for form in ("ascii", "packed"):
            st, _, o = _call(form, s, off, k, np.arange(nq, dtype=np.uint64), END, 0, 3, words=words, woff=woff)
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            if not host:
                assert o.untouched()


@pytest.mark.parametrize("L_", [16, 33, 64, 150])
def test_identity_with_the_fixed_anchored_form_on_equal_lengths(L_):
    free = _free()
    rng = np.random.default_rng(L_)
    count = 9
    for k in sorted({1, 2, min(16, L_), min(31, L_), min(32, L_)}):
        queries = ro.random_queries(rng, 7, k)
        s = ro.random_reads(rng, L_, count, k, queries)
        off = rb.offsets_of([L_] * count)
        words, woff = ro.pack_reads(s, L_, count), rb.word_offsets_of(off)
        last = L_ - k
        for lo, hi in ((0, 0), (0, min(3, last)), (last // 2, min(last // 2 + 5, last)), (max(0, last - 3), last), (last, last + 4)):
            want = free.reads_hdist_anchored(s, L_, k, queries, pos_lo=lo, pos_hi=hi)
            assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=lo, pos_hi=hi, anchor="start"), want), (k, lo, hi)
            assert _same(free.reads_hdist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=lo, pos_hi=hi, anchor="start"),
                         free.reads_hdist_anchored_packed(words, L_, count, k, queries, pos_lo=lo, pos_hi=hi)), (k, lo, hi)
        for e_lo, e_hi in ((0, 0), (0, min(3, last)), (min(2, last), min(7, last)), (last, last)):
            want = free.reads_hdist_anchored(s, L_, k, queries, pos_lo=last - e_hi, pos_hi=last - e_lo)
            assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=e_lo, pos_hi=e_hi, anchor="end"), want), (k, e_lo, e_hi)
            assert _same(free.reads_hdist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=e_lo, pos_hi=e_hi, anchor="end"), want), (k, e_lo, e_hi)


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_identity_with_best_batch_on_reads_of_at_most_64_bases(k):
    free = _free()
    rng = np.random.default_rng(640 + k)
    lengths = list(rng.integers(0, 65, size=40)) + [0, k - 1, k, 64]
    queries = ro.random_queries(rng, 9, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    words, woff = rb.pack_batch(s, off), rb.word_offsets_of(off)
    want = free.reads_hdist_best_batch(s, off, k, queries)
    assert _same(want, rb.batch_best(s, off, k, queries))
    assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=64 - k, anchor="start")[:3], want)
    assert _same(free.reads_hdist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=0, pos_hi=64 - k, anchor="start", second=False), want)
    assert _same(free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=64 - k, anchor="end")[:3], want)  # END over the whole read: the same windows
