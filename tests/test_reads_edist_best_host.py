"""CPU tests of the indel-tolerant best match per read over the WHOLE read (bitnuc_reads_edist_best / _packed / _batch / _batch_packed and the pattern twins):
the host path below the cutoff, through a NULL context, against tests/reads_edist_best_oracle.py (the plain DP of reads_edist_oracle over the whole read; the
host path is the bit-parallel recurrence) -- both layouts, both query kinds; k in {1, 2, 15, 16, 17, 31, 32} x lengths around k and around the 64-base pieces;
planted reads with (dist, end) asserted by hand; ties; all-N, empty-set and singleton patterns; the overhang traps (a copy completed by the next read, the
previous read or the packed pad bits must not score 0); a short read between two long ones; fills; invalid bytes with their absolute index (and none reported
in a read shorter than k); the argument checks in their order; the 2^26 limit judged on the arguments alone; the cutoff on bases x queries; the five
identities of the header; and the host helpers (csrc/reads_edist_best_host.h) under ASan + UBSan in a stand-alone program
(tests/c/reads_edist_best_host_sanitize.cpp).  Every comparison is exact equality of all written arrays; guard words and bytes surround the six outputs,
both dist arrays start at odd byte offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_best_oracle as bo
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL32 = 0x5A5A5A5A
SIZE_MAX = C.c_size_t(-1).value
MAX_READ = 1 << 26  # BITNUC_EDIST_MAX_READ
Q16 = np.array([0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 1, 3])     # ACGTAACCGGTTAGCT
FAR16 = np.array([3] * 15 + [2])                                     # TTTTTTTTTTTTTTTG


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


def _queries(queries, pattern):
    q = rp.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    return q, q.shape[0]


def _fixed(form, s, read_len, count, k, queries, second=True, pattern=False, words=None):
    """the raw fixed-layout entry point with guarded outputs: (status, err, Out)"""
    from bitnuc_amd import _lib as L
    lib = L.load()
    q, nq = _queries(queries, pattern)
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_best"
    o = Out(count)
    if form == "ascii":
        st, e = _raw(getattr(lib, name), None, _p(s), read_len, count, k, _p(q), nq, *o.ptrs(second))
    else:
        words = ro.pack_reads(s, read_len, count) if words is None else words
        st, e = _raw(getattr(lib, name + "_packed"), None, _p(words), read_len, count, k, _p(q), nq, *o.ptrs(second))
    return st, e, o


def _ragged(form, s, off, k, queries, second=True, pattern=False, words=None, woff=None):
    from bitnuc_amd import _lib as L
    lib = L.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count = off.size - 1
    q, nq = _queries(queries, pattern)
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_best_batch"
    o = Out(count)
    if form == "ascii":
        st, e = _raw(getattr(lib, name), None, _p(s), _p(off), count, k, _p(q), nq, *o.ptrs(second))
    else:
        woff = rb.word_offsets_of(off) if woff is None else woff
        words = rb.pack_batch(s, off, seed=k) if words is None else words
        st, e = _raw(getattr(lib, name + "_packed"), None, _p(words), _p(woff), _p(off), count, k, _p(q), nq, *o.ptrs(second))
    return st, e, o


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def _plant(rng, s, off, k, queries, share=0.8):
    """a copy of a query with 1 .. 3 edits, at least one of them an indel, anywhere inside about `share` of the reads of at least k + 3 bases"""
    lens = np.diff(off.astype(np.int64))
    for r in np.nonzero(lens >= k + 3)[0]:
        if rng.random() >= share:
            continue
        c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, len(queries)))], k), int(rng.integers(1, 4)))
        at = int(off[r]) + int(rng.integers(0, int(lens[r]) - len(c) + 1))
        s[at:at + len(c)] = _ascii(c) | (s[at:at + len(c)] & 0x20)


def test_host_helpers_under_asan_ubsan(tmp_path):
    name = "reads_edist_best_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "reads edist best host ok" in out.stdout


def _lengths(k):
    return [k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 150, 257]


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 31, 32])
def test_host_path_grid_against_the_oracle(k):
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(0xED22 + k)
    lengths = _lengths(k)
    # ragged: every length three times, shuffled, in one batch
    ragged = np.array(lengths * 3)
    rng.shuffle(ragged)
    for nq in (1, 2, 5):
        queries = ro.random_queries(rng, nq, k)
        s, off = rb.random_batch(rng, ragged, k, queries)
        _plant(rng, s, off, k, queries)
        want = bo.reads_edist_best_batch(s, off, k, queries)
        lens = np.diff(off.astype(np.int64))
        assert (want[2][lens < k] == 255).all() and (want[2][lens >= k] <= k).all()
        for form in ("ascii", "packed"):
            for pattern, qq in ((False, queries), (True, rp.singletons(queries, k))):
                st, _, o = _ragged(form, s, off, k, qq, pattern=pattern)
                assert st == L.OK and _same(o.read(), want), (form, pattern, nq)
            st, _, o = _ragged(form, s, off, k, queries, second=False)
            assert st == L.OK and _same(o.read()[:3], want[:3]) and o.untouched(which=(1,))
        assert _same(free.reads_edist_best_batch(s, off, k, queries), want)
        woff, words = rb.word_offsets_of(off), rb.pack_batch(s, off)
        assert _same(free.reads_edist_best_batch_packed(words, woff, off, k, queries), want)
        assert _same(free.reads_pattern_edist_best_batch(s, off, k, rp.singletons(queries, k)), want)
        assert _same(free.reads_pattern_edist_best_batch_packed(words, woff, off, k, rp.singletons(queries, k), second=False), want[:3])
    # fixed: one small batch per length
    queries = ro.random_queries(rng, 3, k)
    for n in lengths:
        count = 4
        s, off = rb.random_batch(rng, [n] * count, k, queries)
        _plant(rng, s, off, k, queries)
        want = bo.reads_edist_best(s, n, count, k, queries)
        assert (want[2] == 255).all() if n < k else (want[2] <= k).all()
        for form in ("ascii", "packed"):
            for pattern, qq in ((False, queries), (True, rp.singletons(queries, k))):
                st, _, o = _fixed(form, s, n, count, k, qq, pattern=pattern)
                assert st == L.OK and _same(o.read(), want), (form, pattern, n)
        if n:
            assert _same(free.reads_edist_best(s, n, k, queries), want)
            assert _same(free.reads_edist_best_packed(ro.pack_reads(s, n, count), n, count, k, queries, second=False), want[:3])
            assert _same(free.reads_pattern_edist_best(s, n, k, rp.singletons(queries, k)), want)
            assert _same(free.reads_pattern_edist_best_packed(ro.pack_reads(s, n, count), n, count, k, rp.singletons(queries, k)), want)


def planted_reads():
    """four reads of 257 G's (the query never aligns cheaply with a run of G) with one planted element each, k = 16, queries (FAR16, Q16):
    0: Q16 with base 5 deleted (15 bases) at 58 .. 72, straddling base 64: dist 1, end 73
    1: Q16 with a T inserted before position 8 (17 bases) at 120 .. 136, the inserted base is base 128: dist 1, end 137
    2: Q16 as the read's last 16 bases: dist 0, end 257
    3: Q16 at base 0: dist 0, end 16"""
    n = 257
    reads = np.full((4, n), 2, dtype=np.int64)
    reads[0, 58:73] = np.delete(Q16, 5)
    reads[1, 120:137] = np.insert(Q16, 8, 3)
    reads[2, n - 16:] = Q16
    reads[3, :16] = Q16
    queries = np.array([ro.word_of(FAR16), ro.word_of(Q16)], dtype=np.uint64)
    return 16, n, _ascii(reads.reshape(-1)), queries, [(1, 73), (1, 137), (0, 257), (0, 16)]


def test_planted_reads_dist_and_end_by_hand():
    from bitnuc_amd import _lib as L
    k, n, s, queries, hand = planted_reads()
    want = bo.reads_edist_best(s, n, 4, k, queries)
    assert [(int(d), int(e)) for d, e in zip(want[2], want[1])] == hand and (want[0] == 1).all() and (want[3] == 0).all()
    off = rb.offsets_of([n] * 4)
    for form in ("ascii", "packed"):
        st, _, o = _fixed(form, s, n, 4, k, queries)
        assert st == L.OK and _same(o.read(), want)
        st, _, o = _ragged(form, s, off, k, queries)
        assert st == L.OK and _same(o.read(), want)


def test_ties_two_ends_two_queries_and_a_duplicate():
    from bitnuc_amd import _lib as L
    k, n = 16, 200
    codes = np.full(n, 2, dtype=np.int64)
    codes[30:46] = Q16
    codes[140:156] = Q16  # two exact copies: the first end wins
    s = _ascii(codes)
    qw = ro.word_of(Q16)
    queries = np.array([ro.word_of(FAR16), qw, qw], dtype=np.uint64)  # a duplicate at a higher index is the runner-up
    want = bo.reads_edist_best(s, n, 1, k, queries)
    assert [int(a[0]) for a in want] == [1, 46, 0, 2, 46, 0]
    for form in ("ascii", "packed"):
        st, _, o = _fixed(form, s, n, 1, k, queries)
        assert st == L.OK and _same(o.read(), want)
        st, _, o = _ragged(form, s, rb.offsets_of([n]), k, queries)
        assert st == L.OK and _same(o.read(), want)
    st, _, o = _fixed("ascii", s, n, 1, k, queries[1:2])  # one query: the fill in the second triple
    assert st == L.OK and [int(a[0]) for a in o.read()] == [0, 46, 0, 0xFFFFFFFF, 0xFFFFFFFF, 255]


def test_patterns_all_n_empty_set_and_singletons():
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(5)
    for k in (1, 16, 32):
        lengths = [k, 70, 0, 129, k - 1, 64]
        queries = ro.random_queries(rng, 2, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        ones = (1 << k) - 1
        all_n = np.array([ones] * 4, dtype=np.uint32)
        empty = np.zeros(4, dtype=np.uint32)
        mixed = rp.singletons(queries, k)
        pats = np.stack([empty, mixed[0], all_n, mixed[1]])
        want = bo.reads_pattern_edist_best_batch(s, off, k, pats)
        lens = np.diff(off.astype(np.int64))
        assert (want[2][lens >= k] == 0).all()  # all-N: distance 0
        for form in ("ascii", "packed"):
            st, _, o = _ragged(form, s, off, k, pats, pattern=True)
            assert st == L.OK and _same(o.read(), want)
            st, _, o = _ragged(form, s, off, k, all_n[None, :], pattern=True)  # matches everywhere: distance 0, first reached at end k
            got = o.read()
            assert st == L.OK and (got[2][lens >= k] == 0).all() and (got[1][lens >= k] == k).all() and (got[2][lens < k] == 255).all()
            st, _, o = _ragged(form, s, off, k, empty[None, :], pattern=True)  # never matches: k edits, first reached at end 1
            got = o.read()
            assert st == L.OK and _same(got, bo.reads_pattern_edist_best_batch(s, off, k, empty[None, :]))
            assert (got[2][lens >= k] == k).all() and (got[1][lens >= k] == 1).all()


def test_overhang_traps_a_copy_completed_outside_the_read_does_not_score_zero():
    """read 1 ends with Q16's first ten bases and read 2 starts with its last six (and the other way round for reads 3 and 4); the packed pad bits of read 1
    hold the last six as well.  An implementation that runs past a read's end, or starts before its start, scores 0."""
    from bitnuc_amd import _lib as L
    k = 16
    lengths = [70, 74, 70, 40, 130]
    codes = [np.full(n, 2, dtype=np.int64) for n in lengths]
    codes[1][-10:] = Q16[:10]
    codes[2][:6] = Q16[10:]
    codes[3][-6:] = Q16[:6]
    codes[4][:10] = Q16[6:]
    s = _ascii(np.concatenate(codes))
    off = rb.offsets_of(lengths)
    queries = np.array([ro.word_of(Q16)], dtype=np.uint64)
    want = bo.reads_edist_best_batch(s, off, k, queries)
    assert (want[2] > 0).all()
    words = rb.pack_batch(s, off, pad_codes={1: list(Q16[10:]), 3: list(Q16[6:])})
    for form in ("ascii", "packed"):
        st, _, o = _ragged(form, s, off, k, queries, words=words)
        assert st == L.OK and _same(o.read(), want)
    # the fixed layout: reads of 74 bases, the copy split across the boundary of reads 0 | 1, pad bits completing read 0's
    n = 74
    f = np.full((3, n), 2, dtype=np.int64)
    f[0, -10:] = Q16[:10]
    f[1, :6] = Q16[10:]
    s = _ascii(f.reshape(-1))
    want = bo.reads_edist_best(s, n, 3, k, queries)
    assert (want[2] > 0).all()
    pad = np.full((3, 96 - n), 2, dtype=np.int64)
    pad[0, :6] = Q16[10:]
    for form, w in (("ascii", None), ("packed", ro.pack_reads(s, n, 3, pad_codes=pad))):
        st, _, o = _fixed(form, s, n, 3, k, queries, words=w)
        assert st == L.OK and _same(o.read(), want)


def test_a_read_shorter_than_k_between_two_long_ones_and_its_bytes_are_not_validated():
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    free = _free()
    rng = np.random.default_rng(8)
    k = 16
    lengths = [150, 15, 200, 0, 3, 64]
    queries = ro.random_queries(rng, 3, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    _plant(rng, s, off, k, queries, share=1.0)
    o_ = [int(x) for x in off]
    want = bo.reads_edist_best_batch(s, off, k, queries)
    assert [int(d) for d in want[2][[1, 3, 4]]] == [255] * 3 and (want[2][[0, 2, 5]] <= k).all()
    b = s.copy()
    b[o_[1]:o_[2]] = ord("N")  # every byte of the reads shorter than k: not reported
    b[o_[4]:o_[5]] = 0
    for form in ("ascii", "packed"):
        st, _, o = _ragged(form, b, off, k, queries, words=rb.pack_batch(s, off))
        assert st == L.OK and _same(o.read(), want)
    # an invalid byte inside a read with a window: its absolute index, the first in buffer order, the outputs untouched
    b[o_[5] + 63] = ord("x")
    b[o_[2] + 64] = ord("n")
    with pytest.raises(bn.NucleotideError) as ei:
        free.reads_edist_best_batch(b, off, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("n"), o_[2] + 64)
    for pattern, qq in ((False, queries), (True, rp.singletons(queries, k))):
        st, e, o = _ragged("ascii", b, off, k, qq, pattern=pattern)
        assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("n"), o_[2] + 64) and o.untouched()
    b[o_[2] + 64] = s[o_[2] + 64]
    st, e, o = _ragged("ascii", b, off, k, queries)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("x"), o_[5] + 63) and o.untouched()
    # the fixed layout: every byte of every read
    n, count = 70, 3
    f, _ = rb.random_batch(rng, [n] * count, k, queries)
    f[2 * n + 69] = ord("-")
    st, e, o = _fixed("ascii", f, n, count, k, queries)
    assert st == L.INVALID_BASE and (e.byte, e.index) == (ord("-"), 2 * n + 69) and o.untouched()
    st, _, o = _fixed("ascii", f, 15, 14, k, queries)  # read_len < k: fills, nothing read or validated
    assert st == L.OK and _same(o.read(), eo.fill6(14))


def test_fills_no_query_k_zero_and_count_zero():
    from bitnuc_amd import _lib as L
    s = _ascii(np.zeros(64, dtype=np.int64))
    q = np.zeros(2, dtype=np.uint64)
    for k, nq, n in ((0, 2, 16), (5, 0, 16), (17, 2, 16)):
        for form in ("ascii", "packed"):
            st, _, o = _fixed(form, s, n, 4, k, q[:nq])
            assert st == L.OK and _same(o.read(), eo.fill6(4))
            st, _, o = _ragged(form, s, rb.offsets_of([n] * 4), k, q[:nq])
            assert st == L.OK and _same(o.read(), eo.fill6(4))
    for form in ("ascii", "packed"):
        st, _, o = _fixed(form, s, 16, 0, 5, q)
        assert st == L.OK and o.untouched()
        st, _, o = _ragged(form, s, rb.offsets_of([]), 5, q)
        assert st == L.OK and o.untouched()


def test_argument_checks_and_their_order():
    from bitnuc_amd import _lib as L
    lib = L.load()
    s = np.frombuffer(b"ACGT" * 64, dtype=np.uint8).copy()
    sp = _p(s)
    words = np.zeros(9, dtype=np.uint64)
    wp = _p(words)
    off = rb.offsets_of([64, 64, 64, 64])
    woff = rb.word_offsets_of(off)
    q = np.zeros(32, dtype=np.uint64)  # eight patterns as well (all sets empty)
    qp = _p(q)
    none6 = (None,) * 6
    bad_tab = C.c_void_p(off.ctypes.data + 4)
    decreasing = np.array([0, 9, 3, 3, 3], dtype=np.uint64)
    for kind, qalign in (("", 4), ("pattern_", 2)):
        fx, fxp = getattr(lib, f"bitnuc_reads_{kind}edist_best"), getattr(lib, f"bitnuc_reads_{kind}edist_best_packed")
        rg, rgp = getattr(lib, f"bitnuc_reads_{kind}edist_best_batch"), getattr(lib, f"bitnuc_reads_{kind}edist_best_batch_packed")
        o = Out(8)
        outs = o.ptrs()
        # 1. the _async forms check the context first, whatever else is wrong
        for name, head in (("", (None, 2**40, 2**40)), ("_packed", (None, 2**40, 2**40)), ("_batch", (None, None, 2**40, 2**60)),
                           ("_batch_packed", (None, None, None, 2**40, 2**60))):
            st, e = _raw(getattr(lib, f"bitnuc_reads_{kind}edist_best{name}_async"), None, *head, 40, None, 70000, *none6)
            assert st == L.UNSUPPORTED and e.value == 0
        # 2. k > 32 first, with everything else wrong as well
        for fn, head in ((fx, (None, 2**40, 2**40)), (fxp, (None, 2**40, 2**40)), (rg, (None, None, 2**40)), (rgp, (None, None, None, 2**40))):
            st, e = _raw(fn, None, *head, 33, None, 70000, *none6)
            assert st == L.SEQUENCE_TOO_LONG and e.value == 33
        # 3. fixed: the read_len / count limits (value = read_len), before the query limit
        for fn in (fx, fxp):
            st, e = _raw(fn, None, None, 2**32 - 1, 1, 5, None, 70000, *none6)
            assert st == L.UNSUPPORTED and e.value == 2**32 - 1
            st, e = _raw(fn, None, None, 1 << 20, 1 << 38, 5, None, 70000, *none6)
            assert st == L.UNSUPPORTED and e.value == 1 << 20
        # 4. too many queries, before the read-length bound, count == 0 and the pointers
        for fn, head in ((fx, (None, MAX_READ + 1, 0)), (fxp, (None, MAX_READ + 1, 0)), (rg, (None, None, 0)), (rgp, (None, None, None, 0))):
            st, e = _raw(fn, None, *head, 5, None, 65537, *none6)
            assert st == L.UNSUPPORTED and e.value == 65537
        # 5. fixed: read_len above 2^26 (value = read_len), on the arguments alone: before count == 0 and with a 1-byte buffer
        one = np.zeros(1, dtype=np.uint8)
        for fn in (fx, fxp):
            st, e = _raw(fn, None, None, MAX_READ + 1, 0, 5, None, 3, *none6)
            assert st == L.UNSUPPORTED and e.value == MAX_READ + 1
            st, e = _raw(fn, None, _p(one), MAX_READ + 1, 1, 5, qp, 3, *outs)
            assert st == L.UNSUPPORTED and e.value == MAX_READ + 1
        # 6. count == 0: OK, nothing written, with NULL everywhere
        for fn, head in ((fx, (None, 64, 0)), (fxp, (None, 64, 0)), (rg, (None, None, 0)), (rgp, (None, None, None, 0))):
            st, e = _raw(fn, None, *head, 5, None, 3, *none6)
            assert st == L.OK
        # 7. the pointers: a best output NULL, the second triple partly NULL, misaligned query / end arrays, queries NULL or misaligned, tables NULL or
        # misaligned -- before the tables are read (they are invalid) and before the fill
        def shifted(i, by):
            return tuple(C.c_void_p(p.value + by) if j == i else p for j, p in enumerate(outs))
        bad = [(qp, tuple(None if j == i else p for j, p in enumerate(outs))) for i in range(6)]
        bad += [(qp, tuple(None if j in pair else p for j, p in enumerate(outs))) for pair in ((3, 4), (3, 5), (4, 5), (0, 3, 4, 5))]
        bad += [(None, outs), (C.c_void_p(q.ctypes.data + qalign), outs)]
        bad += [(qp, shifted(0, 2)), (qp, shifted(1, 1)), (qp, shifted(3, 2)), (qp, shifted(4, 1))]
        for qq, six in bad:
            for fn, head in ((fx, (sp, 64, 4)), (fxp, (wp, 64, 4)), (rg, (sp, _p(decreasing), 4)), (rgp, (wp, _p(decreasing), _p(decreasing), 4))):
                st, e = _raw(fn, None, *head, 5, qq, 2, *six)
                assert st == L.UNSUPPORTED and e.value == 0
        for fn, head in ((rg, (sp, None, 4)), (rg, (sp, bad_tab, 4)), (rgp, (wp, None, _p(off), 4)), (rgp, (wp, _p(woff), None, 4)), (rgp, (wp, bad_tab, _p(off), 4)),
                         (rgp, (wp, _p(woff), bad_tab, 4))):
            st, e = _raw(fn, None, *head, 5, qp, 2, *outs)
            assert st == L.UNSUPPORTED and e.value == 0
        # 8. ragged: the tables' faults, then a read above 2^26 bases (value = its length): both before the fill and before the data pointer is looked at
        for fn, head in ((rg, (None, _p(decreasing), 4)), (rgp, (None, _p(decreasing), _p(decreasing), 4))):
            st, e = _raw(fn, None, *head, 0, qp, 0, *outs)
            assert st == L.INVALID_RANGE and e.value == 2
        long_tab = np.array([0, MAX_READ + 1], dtype=np.uint64)
        for fn, head in ((rg, (None, _p(long_tab), 1)), (rgp, (None, _p(rb.word_offsets_of(long_tab)), _p(long_tab), 1))):
            st, e = _raw(fn, None, *head, 5, qp, 2, *outs)
            assert st == L.UNSUPPORTED and e.value == MAX_READ + 1
            st, e = _raw(fn, None, *head, 0, qp, 0, *outs)  # also where the call would write only fills
            assert st == L.UNSUPPORTED and e.value == MAX_READ + 1
        ok_tab = np.array([0, MAX_READ], dtype=np.uint64)  # 2^26 itself is allowed: the next check (NULL data) answers
        st, e = _raw(rg, None, None, _p(ok_tab), 1, 5, qp, 2, *outs)
        assert st == L.UNSUPPORTED and e.value == 0
        assert o.untouched()
        # 9. no window: the fill, before the data is looked at (NULL)
        for fn, head in ((fx, (None, 4, 4)), (fxp, (None, 4, 4)), (rg, (None, _p(rb.offsets_of([1, 0, 1, 1])), 4)),
                         (rgp, (None, _p(rb.word_offsets_of(rb.offsets_of([1, 0, 1, 1]))), _p(rb.offsets_of([1, 0, 1, 1])), 4))):
            o4 = Out(4)
            st, _ = _raw(fn, None, *head, 5, qp, 8, *o4.ptrs())
            assert st == L.OK and _same(o4.read(), eo.fill6(4))
        # 10. then NULL data, or packed words not 8-byte aligned
        o4 = Out(4)
        for fn, head in ((fx, (None, 64, 4)), (fxp, (None, 64, 4)), (fxp, (C.c_void_p(words.ctypes.data + 4), 64, 4)), (rg, (None, _p(off), 4)),
                         (rgp, (None, _p(woff), _p(off), 4)), (rgp, (C.c_void_p(words.ctypes.data + 4), _p(woff), _p(off), 4))):
            st, _ = _raw(fn, None, *head, 5, qp, 8, *o4.ptrs())
            assert st == L.UNSUPPORTED
        assert o4.untouched()
    # and a valid call: AAAAA (three equal queries) against ACGTACGT...: ACGTA has both its A's in place, three substitutions, first reached at end 5
    o = Out(4)
    st, _ = _raw(lib.bitnuc_reads_edist_best, None, sp, 64, 4, 5, qp, 3, *o.ptrs())
    got = o.read()
    assert st == L.OK and _same(got, bo.reads_edist_best(s, 64, 4, 5, q[:3]))
    assert [list(a) for a in got] == [[0] * 4, [5] * 4, [3] * 4, [1] * 4, [5] * 4, [3] * 4]


def test_host_cutoff_is_judged_on_the_bases_of_reads_with_a_window_times_queries():
    """Below the cutoff (1 Mi bases x queries) the host forms need no context; above it they do (a NULL context -> Unsupported).  Fixed: count x read_len.
    Ragged: only the reads of at least k bases count -- 5000 reads of 19 bases among 20000 of 15."""
    from bitnuc_amd import _lib as L
    k = 16
    rng = np.random.default_rng(1)
    s = ro.LUT[rng.integers(0, 4, size=5000 * 19)].astype(np.uint8)  # 95,000 bases; x 11 < 2^20 <= x 12
    lengths = np.array([19] * 5000 + [15] * 20000)
    rng.shuffle(lengths)
    off = rb.offsets_of(lengths)
    b = ro.LUT[rng.integers(0, 4, size=int(off[-1]))].astype(np.uint8)
    woff, words = rb.word_offsets_of(off), rb.pack_batch(b, off)
    for nq, host in ((11, True), (12, False)):
        for form in ("ascii", "packed"):
            st, _, o = _fixed(form, s, 19, 5000, k, np.arange(nq, dtype=np.uint64))
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            assert host or o.untouched()
            st, _, o = _ragged(form, b, off, k, np.arange(nq, dtype=np.uint64), words=words, woff=woff)
            assert st == (L.OK if host else L.UNSUPPORTED), nq
            assert host or o.untouched()


@pytest.mark.parametrize("n", [16, 33, 64])
def test_identity_with_the_anchored_form_on_reads_of_at_most_64_bases(n):
    free = _free()
    rng = np.random.default_rng(n)
    k, count = 16, 40
    queries = ro.random_queries(rng, 4, k)
    s, off = rb.random_batch(rng, [n] * count, k, queries)
    _plant(rng, s, off, k, queries)
    w = ro.pack_reads(s, n, count)
    assert _same(free.reads_edist_best(s, n, k, queries), free.reads_edist_anchored(s, n, k, queries, pos_lo=0, pos_hi=None))
    assert _same(free.reads_edist_best_packed(w, n, count, k, queries), free.reads_edist_anchored_packed(w, n, count, k, queries, pos_lo=0, pos_hi=None))


def test_identities_ragged_equals_fixed_hamming_bound_and_truncation():
    free = _free()
    rng = np.random.default_rng(77)
    k, n, count = 16, 150, 60
    queries = ro.random_queries(rng, 5, k)
    s, off = rb.random_batch(rng, [n] * count, k, queries)
    _plant(rng, s, off, k, queries)
    fixed = free.reads_edist_best(s, n, k, queries)
    assert _same(free.reads_edist_best_batch(s, off, k, queries), fixed)
    assert _same(free.reads_edist_best_batch_packed(rb.pack_batch(s, off), rb.word_offsets_of(off), off, k, queries), fixed)
    assert _same(free.reads_pattern_edist_best(s, n, k, rp.singletons(queries, k)), fixed)
    ham = free.reads_hdist_best(s, n, k, queries)
    assert (fixed[2] <= ham[2]).all() and (fixed[2] < ham[2]).any()
    assert (fixed[2] <= bo.hamming_best_dist(s, off, k, queries)).all()
    for m in (k, 63, 64, 65, 128, 149):
        cut = np.ascontiguousarray(s.reshape(count, n)[:, :m]).reshape(-1)
        assert (free.reads_edist_best(cut, m, k, queries)[2] >= fixed[2]).all(), m


def test_the_long_read_oracle_is_the_plain_dp():
    rng = np.random.default_rng(3)
    for k in (1, 16, 32):
        pats = rp.singletons(ro.random_queries(rng, 3, k), k)
        codes = rng.integers(0, 4, size=300)
        d, j = bo.long_read_columns(codes, k, pats)
        d0, j0 = eo.edist_columns(codes[None, :], k, pats)
        assert np.array_equal(d, d0[:, 0]) and np.array_equal(j, j0[:, 0])
