"""CPU tests of the indel-tolerant anchored match per read of a ragged batch (bitnuc_reads_edist_anchored_batch / _packed and the pattern twins): the host
path below the cutoff, through a NULL context, against tests/reads_edist_batch_oracle.py (the ragged Hamming oracle's windows, the plain DP on each read's
own span; the host path is the bit-parallel recurrence) -- both anchors, both layouts, both query kinds; lengths that give every number of admissible
offsets, 0 included; k in {1, 2, 16, 31, 32} with the widest spans k .. 64; the overhang traps (a copy of a query completed by the next read's first bases,
by the previous read's last bases, by the packed pad bits: it must not score 0) and a planted indel copy exactly filling a short span; the planted cases of
reads_edist_oracle in reads of different lengths; ties; all-N, empty-set and singleton patterns; fills and count == 0; span 64 accepted, 65 and SIZE_MAX
Unsupported with their value; invalid bytes inside a span with their absolute index and the outputs untouched, outside ignored; the argument checks in
their documented order; the cutoff judged on count x the widest span x n_queries; the identities with the fixed form on equal lengths and the
<= -Hamming inequality; and the host helpers (csrc/reads_edist_host.h) under ASan + UBSan in a stand-alone program
(tests/c/reads_edist_batch_host_sanitize.cpp).  Every comparison is exact equality of all written arrays; guard words and bytes surround the six outputs,
both dist arrays start at odd byte offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pattern_oracle as po
import reads_anchored_batch_oracle as rab
import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_batch_oracle as ebo
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
SIZE_MAX = C.c_size_t(-1).value
START, END = rab.START, rab.END


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
    """the six outputs inside guarded host buffers: GUARD words around query / end, the dist arrays at byte offsets 1 and 3 of theirs"""

    def __init__(self, count):
        self.count = count
        self.w = [np.full(count + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(4)]  # best_query, best_end, second_query, second_end
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
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / end written outside [0, count)"
        for a, off in zip(self.d, (1, 3)):
            assert (a[:off] == 0x5A).all() and (a[off + n:] == 0x5A).all(), "dist written outside [0, count)"
        w = [a[GUARD:GUARD + n].copy() for a in self.w]
        return w[0], w[1], self.d[0][1:1 + n].copy(), w[2], w[3], self.d[1][3:3 + n].copy()


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, second=True, words=None, woff=None, pattern=False):
    """the raw entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count = off.size - 1
    q = rp.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    nq = q.shape[0]
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_anchored_batch"
    o = Out(count)
    if form == "ascii":
        st, e = _raw(getattr(lib, name), None, _p(s), _p(off), count, k, anchor, pos_lo, pos_hi, _p(q), nq, *o.ptrs(second))
    else:
        woff = rb.word_offsets_of(off) if woff is None else woff
        words = rb.pack_batch(s, off, seed=k) if words is None else words
        st, e = _raw(getattr(lib, name + "_packed"), None, _p(words), _p(woff), _p(off), count, k, anchor, pos_lo, pos_hi, _p(q), nq, *o.ptrs(second))
    return st, e, o


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def _plant_in_spans(rng, s, off, k, queries, anchor, pos_lo, pos_hi, share=0.8):
    """a copy of a query with 1 .. 3 edits, at least one of them an indel, inside the span of about `share` of the reads whose span has >= k + 1 bases"""
    first, n = rab.windows(np.diff(off.astype(np.int64)), k, anchor, pos_lo, pos_hi)
    for r in np.nonzero(n >= 2)[0]:
        if rng.random() >= share:
            continue
        span = int(n[r]) + k - 1
        c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, len(queries)))], k), int(rng.integers(1, 4)))[:span]
        at = int(off[r]) + int(first[r]) + int(rng.integers(0, span - len(c) + 1))
        s[at:at + len(c)] = _ascii(c)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_edist_batch_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads edist batch host ok" in out.stdout


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_host_path_grid_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0xED18 + k)
    for width in (1, 2, 4, 64 - k + 1):
        for pos_lo in (0, 5):
            pos_hi = pos_lo + width - 1
            lengths = rab.lengths_all_n(k, pos_lo, width)
            rng.shuffle(lengths)
            for nq in (1, 2, 9):
                queries = ro.random_queries(rng, nq, k)
                s, off = rb.random_batch(rng, lengths, k, queries)
                for anchor in (START, END):
                    b = s.copy()
                    _plant_in_spans(rng, b, off, k, queries, anchor, pos_lo, pos_hi)
                    woff, words = rb.word_offsets_of(off), rb.pack_batch(b, off, seed=width)
                    want = ebo.reads_edist_batch(b, off, k, queries, anchor, pos_lo, pos_hi)
                    first, n = rab.windows(np.diff(off.astype(np.int64)), k, anchor, pos_lo, pos_hi)
                    assert set(range(width + 1)) <= set(n.tolist())  # every number of admissible offsets, 0 included
                    has = n > 0
                    assert ((want[2] == 0xFF) == ~has).all() and (want[1][has] > first[has]).all() and (want[1][has] <= (first + n + k - 1)[has]).all()
                    for form in ("ascii", "packed"):
                        st, _, o = _call(form, b, off, k, queries, anchor, pos_lo, pos_hi, words=words, woff=woff)
                        assert st == L.OK and _same(o.read(), want), (form, k, width, pos_lo, nq, anchor)
                        st, _, o = _call(form, b, off, k, queries, anchor, pos_lo, pos_hi, second=False, words=words, woff=woff)  # the best triple only
                        assert st == L.OK and _same(o.read()[:3], want[:3]) and o.untouched(which=(1,)), (form, k, width, pos_lo, nq, anchor)
                        st, _, o = _call(form, b, off, k, rp.singletons(queries, k), anchor, pos_lo, pos_hi, words=words, woff=woff, pattern=True)
                        assert st == L.OK and _same(o.read(), want), ("singletons", form, k, width, pos_lo, nq, anchor)
            got = free.reads_edist_anchored_batch(b, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end")  # the numpy wrappers
            assert _same(got, want)
            assert _same(free.reads_edist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end"), want)
            assert _same(free.reads_edist_anchored_batch(b, off, k, queries, pos_lo=pos_lo, pos_hi=pos_hi, anchor=1, second=False), want[:3])
            sing = rp.singletons(queries, k)
            assert _same(free.reads_pattern_edist_anchored_batch(b, off, k, sing, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end"), want)
            assert _same(free.reads_pattern_edist_anchored_batch_packed(words, woff, off, k, sing, pos_lo=pos_lo, pos_hi=pos_hi, anchor="end"), want)


def test_overhang_traps_a_copy_completed_outside_a_short_span_does_not_score_zero():
    """START 0 .. 4, k = 8 (the full span: 12 bases).  Read 0 has 10 bases and ends in the query's first 6; read 1 begins with the query's last 2: a
    matcher that runs into the next read sees a perfect copy.  The END mirror: read 3 (10 bases < k + pos_hi) begins with the query's last 6, read 2 ends in
    its first 2.  Packed: the pad bits behind a short read complete the copy.  And an indel copy (one base deleted: 7 bases) exactly filling a span."""
    from bitnuc_amd import _lib as L
    k = 8
    q = np.array([0, 1, 2, 3, 3, 2, 1, 0])
    g = 2
    r0 = np.r_[[g] * 4, q[:6]]                  # 10 bases, the copy's first six at its end
    r1 = np.r_[q[6:], [g] * 18]                 # 20 bases, begins with the copy's last two
    r2 = np.r_[[g] * 18, q[:2]]                 # ends in the copy's first two
    r3 = np.r_[q[2:], [g] * 4]                  # 10 bases, begins with the copy's last six
    r4 = np.delete(q, 3)                        # 7 bases < k: no window at all, although the next read would complete it
    r5 = np.r_[q[7:], [g] * 11]
    reads = [r0, r1, r2, r3, r4, r5]
    s = _ascii(np.concatenate(reads))
    off = rb.offsets_of([len(r) for r in reads])
    queries = np.array([ro.word_of(q)], dtype=np.uint64)
    # the pad bits of every read's last word continue the copy where the next read does (and junk elsewhere)
    pads = {0: list(q[6:]), 2: list(q[2:]), 3: list(q[6:]), 4: list(q[7:])}
    words = rb.pack_batch(s, off, pad_codes=pads, seed=3)
    woff = rb.word_offsets_of(off)
    for anchor in (START, END):
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, 0, 4)
        assert want[2][0] == 2 and want[2][3] == 2 and want[2][4] == 0xFF, want  # six of eight bases: two edits, never 0; no window in r4
        for form in ("ascii", "packed"):
            st, _, o = _call(form, s, off, k, queries, anchor, 0, 4, words=words, woff=woff)
            assert st == L.OK and _same(o.read(), want), (form, anchor)
    # a copy with one base deleted exactly filling a short span: END 0 .. 0 on a read of k bases whose last k - 1 bases are the copy
    reads = [np.r_[[g], np.delete(q, 3)], np.r_[[g] * 30]]
    s = _ascii(np.concatenate(reads))
    off = rb.offsets_of([len(r) for r in reads])
    for anchor in (START, END):
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, 0, 3)
        assert (int(want[2][0]), int(want[1][0])) == (1, k)
        for form in ("ascii", "packed"):
            st, _, o = _call(form, s, off, k, queries, anchor, 0, 3)
            assert st == L.OK and _same(o.read(), want), (form, anchor)


def test_planted_cases_in_reads_of_different_lengths():
    """the five reads of reads_edist_oracle.planted_cases(), cut to different lengths behind the planted copy, END anchored on the span's last bases"""
    from bitnuc_amd import _lib as L
    k, read_len, lo, n, s, queries = eo.planted_cases()
    cut = (40, 45, 52, 60, 33)  # each keeps the copy (bases 14 .. 31 at most) whole
    reads = [s[r * read_len:r * read_len + c] for r, c in enumerate(cut)]
    b = np.concatenate(reads)
    off = rb.offsets_of(cut)
    want = ebo.reads_edist_batch(b, off, k, queries, START, lo, lo + n - k)
    assert list(want[0]) == [1] * 5 and list(want[2]) == [1, 1, 1, 2, 0] and list(want[1]) == [29, 31, 30, 30, 30]
    assert list(rab.windows(cut, k, START, lo, lo + n - k)[1]) == [15, 15, 15, 15, 8]  # the last read has a shortened span
    for form in ("ascii", "packed"):
        st, _, o = _call(form, b, off, k, queries, START, lo, lo + n - k)
        assert st == L.OK and _same(o.read(), want), form
        st, _, o = _call(form, b, off, k, rp.singletons(queries, k), START, lo, lo + n - k, pattern=True)
        assert st == L.OK and _same(o.read(), want), form
    ham = rab.reads_anchored_batch(b, off, k, queries, START, lo, lo + n - k)
    assert (want[2] <= ham[2]).all() and (want[2][:2] < ham[2][:2]).all()
    want = ebo.reads_edist_batch(b, off, k, queries, END, 0, 14)  # the last 30 bases of every read: ends counted from the read's start
    for form in ("ascii", "packed"):
        st, _, o = _call(form, b, off, k, queries, END, 0, 14)
        assert st == L.OK and _same(o.read(), want), form
    assert list(want[1][[0, 4]]) == [29, 30] and list(want[2][[0, 4]]) == [1, 0]


def test_ties_two_ends_two_queries_and_a_duplicate():
    free = _free()
    k = 6
    q = np.array([0, 1, 2, 3, 1, 0])
    codes = np.full(40, 2)
    codes[5:11], codes[20:26] = q, q                                          # the same distance at two ends: the smaller end
    s = np.concatenate([_ascii(codes), _ascii(codes[:30]), _ascii(codes[8:])])  # 40, 30 and 32 bases
    off = rb.offsets_of([40, 30, 32])
    far = ro.word_of([3] * k)
    queries = np.array([far, ro.word_of(q), far, ro.word_of(q) | (1 << 40)], dtype=np.uint64)  # 3: an equal duplicate of 1 (junk above 2k differs)
    got = free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=58 - k, anchor="start")
    assert _same(got, ebo.reads_edist_batch(s, off, k, queries, START, 0, 58 - k))
    assert [tuple(int(a[r]) for a in got) for r in range(3)] == [(1, 11, 0, 3, 11, 0), (1, 11, 0, 3, 11, 0), (1, 18, 0, 3, 18, 0)]
    got = free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=14, anchor="end")  # the last 20 bases of each read
    assert _same(got, ebo.reads_edist_batch(s, off, k, queries, END, 0, 14))
    assert tuple(int(a[0]) for a in got) == (1, 26, 0, 3, 26, 0) and int(got[1][2]) == 18
    near = q.copy()
    near[2] = 0
    queries = np.array([ro.word_of(near), far, ro.word_of(near)], dtype=np.uint64)  # two queries at the same distance: the smaller index, the other second
    got = free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=30, anchor="start")
    assert _same(got, ebo.reads_edist_batch(s, off, k, queries, START, 0, 30)) and tuple(int(a[0]) for a in got) == (0, 11, 1, 2, 11, 1)
    got = free.reads_edist_anchored_batch(s, off, k, queries[:1], pos_lo=0, pos_hi=30)  # one query: the fill in the second triple
    assert tuple(int(a[0]) for a in got) == (0, 11, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF)


def test_patterns_all_n_empty_set_and_singletons():
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0x9A7)
    for k, lo, hi in ((1, 3, 9), (12, 7, 30), (32, 0, 32)):
        lengths = rab.lengths_all_n(k, lo, hi - lo + 1)
        queries = ro.random_queries(rng, 5, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        woff, words = rb.word_offsets_of(off), rb.pack_batch(s, off, seed=k)
        count = len(lengths)
        for anchor in (START, END):
            first, n = rab.windows(lengths, k, anchor, lo, hi)
            has = n > 0
            all_n = po.from_iupac("N" * k)
            got = free.reads_pattern_edist_anchored_batch(s, off, k, [all_n, rp.singletons(queries, k)[0]], pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert (got[0][has] == 0).all() and (got[1][has] == (first + k)[has]).all() and (got[2][has] == 0).all()  # all-N: (0, a_r + k)
            assert (got[2][~has] == 0xFF).all() and (got[5][~has] == 0xFF).all()
            sets = [po.random_sets(rng, k) for _ in range(4)]
            sets[2] = [set() if i == k // 2 else x for i, x in enumerate(sets[2])]  # an empty set never matches
            pats = rp.as_patterns([po.from_sets(x) for x in sets])
            want = ebo.reads_pattern_edist_batch(s, off, k, pats, anchor, lo, hi)
            for form in ("ascii", "packed"):
                st, _, o = _call(form, s, off, k, pats, anchor, lo, hi, words=words, woff=woff, pattern=True)
                assert st == L.OK and _same(o.read(), want), (form, k, anchor)
            empty = rp.as_patterns([po.from_sets([set()] * k)])
            got = free.reads_pattern_edist_anchored_batch_packed(words, woff, off, k, empty, pos_lo=lo, pos_hi=hi, anchor=anchor, second=False)
            assert _same(got, ebo.reads_pattern_edist_batch(s, off, k, empty, anchor, lo, hi)[:3])
            assert (got[2][has] == k).all() and (got[1][has] == (first + 1)[has]).all() and count == got[0].size


def test_never_above_the_ragged_hamming_form():
    free = _free()
    rng = np.random.default_rng(0xBEE)
    for k, lo, hi in ((16, 0, 3), (31, 2, 9), (5, 0, 40)):
        lengths = list(rng.integers(0, 120, size=80))
        queries = ro.random_queries(rng, 12, k)
        s, off = rb.random_batch(rng, lengths, k, queries, plant=12)
        for anchor in ("start", "end"):
            _plant_in_spans(rng, s, off, k, queries, anchor, lo, hi, share=0.5)
            e = free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor)
            h = free.reads_hdist_anchored_batch(s, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert (e[2] <= h[2]).all() and ((e[2] == 0xFF) == (h[2] == 0xFF)).all()
            assert _same(e, ebo.reads_edist_batch(s, off, k, queries, anchor, lo, hi))


def test_fills_empty_ranges_no_query_and_count_zero():
    from bitnuc_amd import _lib as L
    s = np.frombuffer(b"ACGTAC" * 3, dtype=np.uint8).copy()
    off = rb.offsets_of([6, 0, 12])
    for k, queries, pos_lo, pos_hi in ((0, [1, 2], 0, 3), (13, [1, 2], 0, 3), (3, [], 0, 3), (3, [1, 2], 10, 12), (3, [1, 2], 2, 1), (3, [1, 2], SIZE_MAX, SIZE_MAX),
                                       (3, [1, 2], 2**33, 2**33 + 4)):
        for anchor in (START, END):
            for form in ("ascii", "packed"):
                st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi)
                assert st == L.OK and _same(o.read(), eo.fill6(3)), (k, queries, pos_lo, pos_hi)
                st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_hi, second=False)
                assert st == L.OK and _same(o.read()[:3], eo.fill6(3)[:3]) and o.untouched(which=(1,))
            if k <= 32:
                assert _same(ebo.reads_edist_batch(s, off, k, queries, anchor, pos_lo, pos_hi), eo.fill6(3))
    for anchor in (START, END):  # empty reads at the start, in the middle and at the end of a batch: the fill there, answers elsewhere
        off2 = rb.offsets_of([0, 6, 0, 0, 12, 0])
        want = ebo.reads_edist_batch(s, off2, 3, [27, 1], anchor, 0, 2)
        assert list(want[2] == 0xFF) == [True, False, True, True, False, True]
        for form in ("ascii", "packed"):
            st, _, o = _call(form, s, off2, 3, [27, 1], anchor, 0, 2)
            assert st == L.OK and _same(o.read(), want)
    for form in ("ascii", "packed"):
        st, _, o = _call(form, s, rb.offsets_of([]), 3, [1, 2], START, 0, 3)  # count == 0: nothing written
        assert st == L.OK and o.untouched()


def test_span_64_is_accepted_65_and_size_max_are_unsupported_with_their_value():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(64)
    lengths = [150, 70, 64, 63, 10, 0, 90]
    for k in (1, 16, 32):
        queries = ro.random_queries(rng, 3, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        for anchor in (START, END):
            for pos_lo in (0, 6):
                want = ebo.reads_edist_batch(s, off, k, queries, anchor, pos_lo, pos_lo + 64 - k)
                for form in ("ascii", "packed"):
                    st, _, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_lo + 64 - k)
                    assert st == L.OK and _same(o.read(), want), (form, k, anchor, pos_lo)
                    st, e, o = _call(form, s, off, k, queries, anchor, pos_lo, pos_lo + 65 - k)
                    assert st == L.UNSUPPORTED and e.value == 65 and o.untouched()
                    st, e, o = _call(form, s, off, k, [], anchor, pos_lo, pos_lo + 65 - k)  # judged on the arguments alone: also without queries
                    assert st == L.UNSUPPORTED and e.value == 65 and o.untouched()
            for form in ("ascii", "packed"):  # pos_hi = SIZE_MAX is not "to the end" here
                st, e, o = _call(form, s, off, k, queries, anchor, 0, SIZE_MAX)
                assert st == L.UNSUPPORTED and e.value == SIZE_MAX and o.untouched()
                st, e, o = _call(form, s, off, k, queries, anchor, 1, SIZE_MAX)
                assert st == L.UNSUPPORTED and e.value == (SIZE_MAX if k > 1 else SIZE_MAX - 1 + k) and o.untouched()


def test_invalid_bytes_inside_a_span_absolute_index_outside_ignored():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(12)
    k, lo, hi = 7, 2, 5
    lengths = [50, 8, 30, 0, 6, 9, 41, 12, 10]  # 9: a shortened span (bases 2 .. 8); 10: two offsets
    queries = ro.random_queries(rng, 3, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    o = [int(x) for x in off]
    for anchor in (START, END):
        clean = ebo.reads_edist_batch(s, off, k, queries, anchor, lo, hi)
        mask = rab.span_bytes(off, k, anchor, lo, hi)
        b = s.copy()
        b[~mask] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=int((~mask).sum()))  # every byte no span holds, among them the byte
        # directly behind a short read's span (the next read's first) and every byte of the reads without a window (8 and 6 bases)
        assert not mask[o[1]:o[2]].any() and not mask[o[4]:o[5]].any()
        if anchor == START:
            assert mask[o[5] + 8] and not mask[o[6]]  # read 5's span: its bases 2 .. 8, the byte behind it is read 6's first
        else:
            assert mask[o[5] + 6] and not mask[o[5] + 7]  # its bases 0 .. 6
        st, _, out = _call("ascii", b, off, k, queries, anchor, lo, hi)
        assert st == L.OK and _same(out.read(), clean)
        assert _same(free.reads_edist_anchored_batch(b, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor), clean)
        spans = np.nonzero(mask)[0]
        later, bad_at = int(spans[-1]), int(spans[np.searchsorted(spans, o[6])])  # read 6's first span byte; a later one in the last read
        b[later] = ord("x")
        b[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            free.reads_edist_anchored_batch(b, off, k, queries, pos_lo=lo, pos_hi=hi, anchor=anchor)
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        for pattern, qq in ((False, queries), (True, rp.singletons(queries, k))):
            st, e, out = _call("ascii", b, off, k, qq, anchor, lo, hi, pattern=pattern)
            assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("N"), bad_at) and out.untouched()
        b[bad_at] = s[bad_at]
        st, e, out = _call("ascii", b, off, k, queries, anchor, lo, hi)  # the last span byte of the batch
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("x"), later) and out.untouched()
        st, _, out = _call("ascii", b, off, k, queries, anchor, 60, 70)  # no window: nothing is read or validated
        assert st == L.OK and _same(out.read(), eo.fill6(len(lengths)))


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = _p(s)
    words = np.zeros(9, dtype=np.uint64)
    wp = _p(words)
    off = rb.offsets_of([64, 64, 64, 64])
    woff = rb.word_offsets_of(off)
    short = rb.offsets_of([1, 0, 1, 1])  # three bases in all: no window of five
    q = np.zeros(32, dtype=np.uint64)  # eight patterns as well (all sets empty)
    qp = _p(q)
    none6 = (None,) * 6
    bad_tab = C.c_void_p(off.ctypes.data + 4)

    def host(fn, src, tabs, count, k, anchor, lo, hi, qq, nq, six):
        return _raw(fn, None, src, *tabs, count, k, anchor, lo, hi, qq, nq, *six)
    for kind, qalign in (("", 4), ("pattern_", 2)):  # a pointer that breaks the kind's alignment: 8 bytes exact, 4 bytes patterns
        best, packed = getattr(lib, f"bitnuc_reads_{kind}edist_anchored_batch"), getattr(lib, f"bitnuc_reads_{kind}edist_anchored_batch_packed")
        adev, pdev = getattr(lib, f"bitnuc_reads_{kind}edist_anchored_batch_async"), getattr(lib, f"bitnuc_reads_{kind}edist_anchored_batch_packed_async")
        o = Out(8)
        outs = o.ptrs()
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
        # 7. a best output NULL, one or two of the second outputs NULL, a query / end array of either triple misaligned, queries NULL (with queries) or
        # misaligned, a table NULL or not 8-byte aligned -> Unsupported, before the tables are read (they are invalid: check 8) and the no-window case
        def shifted(i, by):
            return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
        bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
        bad += [(qp, tuple(None if j in pair else p for j, p in enumerate(outs))) for pair in ((3, 4), (3, 5), (4, 5), (0, 3, 4, 5))]
        bad += [(None, outs), (C.c_void_p(q.ctypes.data + qalign), outs)]
        bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1)), (qp, shifted(4, 2))]  # (4: second_end)
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
        # 8. the tables' faults, before the no-window case and the NULL data
        for fn, src, tabs in ((best, None, (_p(decreasing),)), (packed, None, (_p(decreasing), _p(decreasing)))):
            st, e = host(fn, src, tabs, 4, 0, START, 0, 3, qp, 0, outs)
            assert st == L.INVALID_RANGE and e.value == 2
        assert o.untouched()
        # 9. no windows: the fill in [0, count) of all six and nothing after, before the data is looked at (NULL); both dist arrays at odd addresses
        for k, tab, nq, qq, lo, hi in ((0, off, 8, qp, 0, 3), (5, short, 8, qp, 0, 3), (5, off, 0, None, 0, 3), (5, off, 8, qp, 4, 3), (5, off, 8, qp, 252, 260)):
            for fn, tabs in ((best, (_p(tab),)), (packed, (_p(rb.word_offsets_of(tab)), _p(tab)))):
                for anchor in (START, END):
                    o4 = Out(4)
                    st, _ = host(fn, None, tabs, 4, k, anchor, lo, hi, qq, nq, o4.ptrs())
                    assert st == L.OK and _same(o4.read(), eo.fill6(4)), (k, nq, lo, hi)
        # 10. then NULL data, or packed words not 8-byte aligned
        o4 = Out(4)
        outs4 = o4.ptrs()
        st, _ = host(best, None, (_p(off),), 4, 5, START, 0, 3, qp, 8, outs4)
        assert st == L.UNSUPPORTED
        st, _ = host(packed, None, (_p(woff), _p(off)), 4, 5, START, 0, 3, qp, 8, outs4)
        assert st == L.UNSUPPORTED
        st, _ = host(packed, C.c_void_p(words.ctypes.data + 4), (_p(woff), _p(off)), 4, 5, START, 0, 3, qp, 8, outs4)
        assert st == L.UNSUPPORTED
        assert o4.untouched()
    # and a valid call writes [0, count) of each output only: AAAAA (queries 0 .. 2, equal) against a span of ACGTACGT...: one A matches, so the distance
    # is 4.  START 1 .. 3: the span CGTACGT (bases 1 .. 7), first reached at its base 4 (CGTA), end = 1 + 4; END 1 .. 3 (last 59): offsets 56 .. 58, the
    # span ACGTACG (bases 56 .. 62): ACGTA has both its A's in place, three substitutions, end = 56 + 5
    best = lib.bitnuc_reads_edist_anchored_batch
    o = Out(4)
    st, _ = host(best, sp, (_p(off),), 4, 5, START, 1, 3, qp, 3, o.ptrs())
    got = o.read()
    assert st == L.OK and _same(got, ebo.reads_edist_batch(s, off, 5, q[:3], START, 1, 3))
    assert [list(a) for a in got] == [[0] * 4, [5] * 4, [4] * 4, [1] * 4, [5] * 4, [4] * 4]
    o = Out(4)
    st, _ = host(best, sp, (_p(off),), 4, 5, END, 1, 3, qp, 3, o.ptrs())
    got = o.read()
    assert st == L.OK and _same(got, ebo.reads_edist_batch(s, off, 5, q[:3], END, 1, 3))
    assert [list(a) for a in got] == [[0] * 4, [61] * 4, [3] * 4, [1] * 4, [61] * 4, [3] * 4]


def test_host_cutoff_is_judged_on_count_times_the_widest_span_times_queries():
    """Below the cutoff (1 Mi span bases x queries) the host forms need no context; above it they do (a NULL context -> Unsupported).  The widest span,
    four offsets + k - 1 = 19 bases, counts for every read, whatever its length."""
    from bitnuc_amd import _lib as L
    count, k = 5000, 16  # 95,000 span bases in all; x 11 < 2^20 <= x 12
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
def test_identity_with_the_fixed_edist_form_on_equal_lengths(L_):
    free = _free()
    rng = np.random.default_rng(L_)
    count = 9
    for k in sorted({1, 2, min(16, L_), min(31, L_), min(32, L_)}):
        queries = ro.random_queries(rng, 7, k)
        s = ro.random_reads(rng, L_, count, k, queries)
        off = rb.offsets_of([L_] * count)
        words, woff = ro.pack_reads(s, L_, count), rb.word_offsets_of(off)
        sing = rp.singletons(queries, k)
        last = L_ - k
        cap = 64 - k  # the widest range a span of 64 allows
        for lo, hi in ((0, 0), (0, min(3, last)), (last // 2, min(last // 2 + 5, last, last // 2 + cap)), (max(0, last - 3), last), (last, last + min(4, cap))):
            want = free.reads_edist_anchored(s, L_, k, queries, pos_lo=lo, pos_hi=hi)
            assert _same(free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=lo, pos_hi=hi, anchor="start"), want), (k, lo, hi)
            assert _same(free.reads_edist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=lo, pos_hi=hi, anchor="start"),
                         free.reads_edist_anchored_packed(words, L_, count, k, queries, pos_lo=lo, pos_hi=hi)), (k, lo, hi)
            assert _same(free.reads_pattern_edist_anchored_batch(s, off, k, sing, pos_lo=lo, pos_hi=hi, anchor="start"), want), (k, lo, hi)
        for e_lo, e_hi in ((0, 0), (0, min(3, last)), (min(2, last), min(7, last)), (last, last)):
            want = free.reads_edist_anchored(s, L_, k, queries, pos_lo=last - e_hi, pos_hi=last - e_lo)
            assert _same(free.reads_edist_anchored_batch(s, off, k, queries, pos_lo=e_lo, pos_hi=e_hi, anchor="end"), want), (k, e_lo, e_hi)
            assert _same(free.reads_edist_anchored_batch_packed(words, woff, off, k, queries, pos_lo=e_lo, pos_hi=e_hi, anchor="end"), want), (k, e_lo, e_hi)
            assert _same(free.reads_pattern_edist_anchored_batch_packed(words, woff, off, k, sing, pos_lo=e_lo, pos_hi=e_hi, anchor="end"), want), (k, e_lo, e_hi)
