"""CPU tests of the indel-tolerant family's second stage -- where the alignment that ends at a given base starts (bitnuc_reads_edist_start[_packed],
_start_batch[_packed], bitnuc_ref_edist_start[_packed] and the pattern twins): the host forms through a NULL context against tests/edist_start_oracle.py
(one full Levenshtein table per candidate substring; the host path is the backward bit-parallel walk).  Both layouts, both query kinds, ASCII and packed;
k in {1, 2, 15, 16, 17, 31, 32}; ends at the floor, around the window bound 2k - 1 and at the read's end; planted reads with a deleted, an inserted or no
base whose alignments are shorter than, longer than and exactly k; hand cases; floor traps; skipped items; the argument checks in their order; all 256 byte
values at every walked position and beside the walked range; every forward host form followed by the start form; and edist_start_host.h under ASan + UBSan
in a stand-alone program (tests/c/edist_start_host_sanitize.cpp).  Every comparison is exact equality; guard words and bytes surround the outputs, dist
starts at an odd byte offset."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edist_start_oracle as so
import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_pattern_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
MARK32 = 0x5A5A5A5A
MARK64 = 0x5A5A5A5A5A5A5A5A
KS = [1, 2, 15, 16, 17, 31, 32]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from bitnuc_amd import build
    build.ensure_built()


def _L():
    from bitnuc_amd import _lib as L
    return L


def _free():
    from bitnuc_amd import api
    return api.context_free()


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


class Out:
    """start inside GUARD words (u32 per read, u64 along a reference), dist at byte offset 1 of a guarded buffer"""

    def __init__(self, n, wide=False):
        self.n, self.dt, self.mark = n, (np.uint64 if wide else np.uint32), (MARK64 if wide else MARK32)
        self.s = np.full(n + 2 * GUARD, self.mark, dtype=self.dt)
        self.d = np.full(1 + n + GUARD, 0x5A, dtype=np.uint8)

    def ptrs(self, with_dist=True):
        return C.c_void_p(self.s.ctypes.data + self.s.itemsize * GUARD), (C.c_void_p(self.d.ctypes.data + 1) if with_dist else None)

    def untouched(self):
        return bool((self.s == self.mark).all() and (self.d == 0x5A).all())

    def read(self, with_dist=True):
        n = self.n
        assert (self.s[:GUARD] == self.mark).all() and (self.s[GUARD + n:] == self.mark).all(), "start written outside [0, n)"
        assert (self.d[:1] == 0x5A).all() and (self.d[1 + n:] == 0x5A).all(), "dist written outside [0, n)"
        if not with_dist:
            assert (self.d == 0x5A).all(), "dist written through a NULL pointer's neighbour"
        return self.s[GUARD:GUARD + n].copy(), self.d[1:1 + n].copy()


def _queries(queries, pattern):
    q = rp.as_patterns(queries) if pattern else np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
    return q, q.shape[0]


def _raw(fn, *args):
    err = _L().BitnucErr()
    return fn(*args, C.byref(err)), err


def call_reads(layout, packed, pattern, s, shape, k, anchor, pos, queries, query, end, with_dist=True, ctx=None):
    """the raw per-read entry point.  shape: read_len (fixed) or the offsets table (ragged).  -> (status, err, Out)"""
    lib = _L().load()
    q, nq = _queries(queries, pattern)
    query = np.ascontiguousarray(query, dtype=np.uint32)
    end = np.ascontiguousarray(end, dtype=np.uint32)
    name = "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_start" + ("_batch" if layout == "ragged" else "") + ("_packed" if packed else "")
    if layout == "fixed":
        count = query.size
        data = ro.pack_reads(s, shape, count) if packed else s
        head = (_p(data), shape, count)
    else:
        off = np.ascontiguousarray(shape, dtype=np.uint64)
        count = off.size - 1
        if packed:
            woff = rb.word_offsets_of(off)
            data = rb.pack_batch(s, off, seed=k)
            head = (_p(data), _p(woff), _p(off), count)
        else:
            data = s
            head = (_p(data), _p(off), count)
    o = Out(count)
    st, e = _raw(getattr(lib, name), ctx, *head, k, anchor, pos, _p(q), nq, _p(query), _p(end), *o.ptrs(with_dist))
    return st, e, o


def call_ref(packed, pattern, s, k, queries, qidx, end, with_dist=True):
    lib = _L().load()
    q, nq = _queries(queries, pattern)
    end = np.ascontiguousarray(end, dtype=np.uint64)
    qidx = None if qidx is None else np.ascontiguousarray(qidx, dtype=np.uint32)
    name = "bitnuc_ref_" + ("pattern_" if pattern else "") + "edist_start" + ("_packed" if packed else "")
    if packed:
        w = ro.pack_reads(s, len(s), 1)
        head = (_p(w), w.size, len(s))
    else:
        head = (_p(s), len(s))
    o = Out(end.size, wide=True)
    st, e = _raw(getattr(lib, name), None, *head, k, _p(q), nq, _p(qidx), _p(end), end.size, *o.ptrs(with_dist))
    return st, e, o


def want_reads(s, off, k, anchor, pos, queries, query, end):
    codes = ro.codes_of(s)
    off = [int(x) for x in off]
    texts = [codes[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    floors = [so.floor_of(len(t), k, anchor, pos) for t in texts]
    start, dist = so.starts(texts, floors, so.masks_of(queries, k), k, query, end)
    return start.astype(np.uint32), dist


def check_all_reads_forms(s, off, k, anchor, pos, queries, query, end, fixed_len=None):
    """every form that can hold the batch (ragged always; fixed when the reads have one length) x ASCII / packed x exact / singleton patterns"""
    want = want_reads(s, off, k, anchor, pos, queries, query, end)
    pats = rp.singletons(queries, k)
    for layout, shape in (("ragged", off),) + ((("fixed", fixed_len),) if fixed_len is not None else ()):
        for packed in (False, True):
            for pattern in (False, True):
                st, e, o = call_reads(layout, packed, pattern, s, shape, k, anchor, pos, pats if pattern else queries, query, end)
                assert st == 0, (layout, packed, pattern, st, e.value)
                got = o.read()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (layout, packed, pattern, k, anchor, pos)
    return want


def test_oracle_tables_side_by_side_equal_the_scalar_tables():
    rng = np.random.default_rng(0x57A27)
    for _ in range(300):
        k = int(rng.integers(1, 9))
        n = int(rng.integers(0, 30))
        t = rng.integers(0, 2 + int(rng.integers(0, 3)), size=n)
        a = int(rng.integers(0, n + 1))
        e = int(rng.integers(a, n + 1))
        m = so.masks_of_query(int(rng.integers(0, 4 ** k)), k)
        start, dist = so.starts([t], [a], m[None, :], k, [0], [e])
        assert so.start_one(m, t, a, e) == (int(dist[0]), int(start[0]))


def test_host_walk_under_asan_ubsan(tmp_path):
    name = "edist_start_host_sanitize"
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "edist start host ok" in out.stdout


@pytest.mark.parametrize("k", KS)
def test_sweep_of_ends_at_the_floor_around_the_window_bound_and_at_the_reads_end(k):
    rng = np.random.default_rng(0x5EE9 + k)
    queries = ro.random_queries(rng, 3, k)
    for anchor, pos in ((0, 0), (0, 3), (1, 0), (1, 2)):
        L = 2 * k + 9 + pos
        a = so.floor_of(L, k, anchor, pos)
        ends = [a, a + 1, a + 2 * k - 2, a + 2 * k - 1, a + 2 * k, L - 1, L]
        count = len(ends) * 3
        s = _ascii(rng.integers(0, 4, size=count * L))
        s[rng.random(s.size) < 0.3] |= 0x20
        for r in range(count):  # a copy of the read's query ends at the item's end where it fits behind the floor
            e, c = ends[r % len(ends)], ro.query_codes(queries[r % 3], k)
            if e - k >= 0:
                s[r * L + e - k:r * L + e] = _ascii(c)
        end = np.array([ends[r % len(ends)] for r in range(count)], dtype=np.uint32)
        query = np.array([r % 3 for r in range(count)], dtype=np.uint32)
        check_all_reads_forms(s, np.arange(count + 1) * L, k, anchor, pos, queries, query, end, fixed_len=L)
        # along a reference: the floor is 0, the same ends around 0 and n
        n = 5 * k + 40
        ref = _ascii(rng.integers(0, 4, size=n))
        at = 2 * k + 5
        ref[at:at + k] = _ascii(ro.query_codes(queries[1], k))
        rends = np.array([0, 1, 2 * k - 2, 2 * k - 1, 2 * k, at + k, n - 1, n], dtype=np.uint64)
        qidx = np.array([1] * len(rends), dtype=np.uint32)
        ws, wd = so.starts([ro.codes_of(ref)] * len(rends), [0] * len(rends), so.masks_of(queries, k), k, qidx, rends, fill=so.FILL64)
        for packed in (False, True):
            for pattern in (False, True):
                st, e, o = call_ref(packed, pattern, ref, k, rp.singletons(queries, k) if pattern else queries, qidx, rends)
                gs, gd = o.read()
                assert st == 0 and np.array_equal(gs, ws) and np.array_equal(gd, wd), (packed, pattern)
        assert int(wd[5]) == 0 and int(ws[5]) == at


def _planted(rng, k, count, queries):
    """reads of 2k + 20 .. 2k + 60 random bases that carry their query once: a third with one base deleted, a third with one base inserted (mid-query, a
    base that differs from both neighbours), a third exact"""
    lens = rng.integers(2 * k + 20, 2 * k + 61, size=count)
    off = rb.offsets_of(lens)
    s = _ascii(rng.integers(0, 4, size=int(off[-1])))
    which = np.arange(count) % len(queries)
    for r in range(count):
        c = [int(x) for x in ro.query_codes(queries[which[r]], k)]
        i = k // 2
        if r % 3 == 0 and k >= 3:
            del c[i]
        elif r % 3 == 1 and k >= 2:
            c.insert(i, next(x for x in range(4) if x != c[i - 1] and x != c[i]))
        at = int(off[r]) + int(rng.integers(5, int(lens[r]) - len(c) - 4))
        s[at:at + len(c)] = _ascii(c)
    return s, off


@pytest.mark.parametrize("k", KS)
def test_planted_reads_shorter_longer_and_exactly_k(k):
    free = _free()
    rng = np.random.default_rng(0x91A47 + k)
    count = 300
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(4)], dtype=np.uint64)
    s, off = _planted(rng, k, count, queries)
    fq, fe, fd = free.reads_edist_best_batch(s, off, k, queries, second=False)
    ws, wd = check_all_reads_forms(s, off, k, 0, 0, queries, fq, fe)
    assert np.array_equal(wd, fd)  # the identity: the forward form's distance
    if k >= 15:  # asserted on the oracle alone
        length = fe.astype(np.int64) - ws.astype(np.int64)
        for share in ((length < k).mean(), (length > k).mean(), (length == k).mean()):
            assert share >= 0.25, ((length < k).mean(), (length > k).mean(), (length == k).mean())


def test_hand_cases():
    # a tie: ACGT against the text ATCGT ending at 5: ATCGT (one inserted base), TCGT (one substituted) and CGT (one deleted) all cost 1 -- the shortest wins
    st, e, o = call_reads("ragged", False, False, np.frombuffer(b"ATCGT", dtype=np.uint8), [0, 5], 4, 0, 0, [ro.word_of([0, 1, 2, 3])], [0], [5])
    assert st == 0 and [int(x[0]) for x in o.read()] == [2, 1]
    for packed in (False, True):
        s = np.frombuffer(b"GATTACAGATTACA", dtype=np.uint8)
        # an all-N pattern of k = 4 matches every base: the last four bases at distance 0; with two bases behind the floor both of them at distance 2
        alln = np.array([[15, 15, 15, 15]], dtype=np.uint32)
        st, e, o = call_reads("fixed", packed, True, s, 14, 4, 0, 0, alln, [0], [9])
        assert st == 0 and [int(x[0]) for x in o.read()] == [5, 0]
        st, e, o = call_reads("fixed", packed, True, s, 14, 4, 0, 7, alln, [0], [9])
        assert st == 0 and [int(x[0]) for x in o.read()] == [7, 2]
        # empty sets match nothing: every substring of c bases costs max(3, c): the empty one wins, dist = k, start = end
        none = np.zeros((1, 4), dtype=np.uint32)
        st, e, o = call_reads("fixed", packed, True, s, 14, 3, 0, 0, none, [0], [9])
        assert st == 0 and [int(x[0]) for x in o.read()] == [9, 3]
        # dist = k with start = end under an exact query: AAAA in a text of C
        st, e, o = call_reads("fixed", packed, False, np.frombuffer(b"CCCCCCCC", dtype=np.uint8), 8, 4, 0, 0, [0], [0], [5])
        assert st == 0 and [int(x[0]) for x in o.read()] == [5, 4]
        st, e, o = call_ref(packed, False, np.frombuffer(b"CCCCCCCC", dtype=np.uint8), 4, [0], None, [5, 0])
        assert st == 0 and [x.tolist() for x in o.read()] == [[5, 0], [4, 4]]


@pytest.mark.parametrize("k", [2, 16, 31])
def test_floor_traps(k):
    rng = np.random.default_rng(0xF100 + k)
    qc = rng.permutation(np.arange(k) % 4)
    queries = np.array([ro.word_of(qc)], dtype=np.uint64)
    h = k // 2
    # ragged: the copy's first half is the END of the previous read, its second half the start of this one
    lens = [40, 40, k + 1, 3, 40]
    off = rb.offsets_of(lens)
    s = np.full(int(off[-1]), ord("T") if qc[0] != 3 else ord("G"), dtype=np.uint8)
    s[40 - h:40 - h + k] = _ascii(qc)
    end = np.array([40, k - h, k + 1, 3, 12], dtype=np.uint32)
    ws, wd = check_all_reads_forms(s, off, k, 0, 0, queries, np.zeros(5, dtype=np.uint32), end)
    assert int(wd[1]) >= h and int(ws[1]) >= 0  # the h bases in the previous read are not used
    # fixed: the copy's first half lies in front of pos
    L, pos = 70, 20
    s = np.full(3 * L, ord("T") if qc[0] != 3 else ord("G"), dtype=np.uint8)
    for r in range(3):
        s[r * L + pos - h:r * L + pos - h + k] = _ascii(qc)
    end = np.array([pos + k - h] * 3, dtype=np.uint32)
    ws, wd = check_all_reads_forms(s, np.arange(4) * L, k, 0, pos, queries, np.zeros(3, dtype=np.uint32), end, fixed_len=L)
    assert (wd >= h).all() and (ws >= pos).all()
    ws0, wd0 = check_all_reads_forms(s, np.arange(4) * L, k, 0, 0, queries, np.zeros(3, dtype=np.uint32), end, fixed_len=L)
    assert (wd0 == 0).all() and (ws0 == pos - h).all()
    # ragged END floors with len < k + pos: the floor saturates at 0
    pos = 5
    lens = [k + pos - 1, k + pos, k + pos + 1, k, k - 1, 0, 1]
    off = rb.offsets_of(lens)
    s = _ascii(rng.integers(0, 4, size=int(off[-1])))
    for r, ln in enumerate(lens):
        if ln >= k:
            s[int(off[r]):int(off[r]) + k] = _ascii(qc)
    for ends in (lens, [min(ln, k) for ln in lens], [0] * len(lens), [max(0, ln - k - pos) for ln in lens]):
        check_all_reads_forms(s, off, k, 1, pos, queries, np.zeros(len(lens), dtype=np.uint32), np.array(ends, dtype=np.uint32))


def test_skipped_items_write_fills_and_read_nothing():
    k, L = 8, 30
    rng = np.random.default_rng(0x5C19)
    queries = ro.random_queries(rng, 2, k)
    pos = 4
    query = np.array([2, 0xFFFFFFFF, 0, 0, 0xA5A5A5A5, 1, 0], dtype=np.uint32)
    end = np.array([10, 10, L + 1, pos - 1, 0xA5A5A5A5, 12, 0xA5A5A5A5], dtype=np.uint32)
    count = query.size
    s = _ascii(rng.integers(0, 4, size=count * L))
    for r in (0, 1, 2, 3, 4, 6):
        s[r * L:(r + 1) * L] = ord("N")  # a read of a skipped item would be an invalid base
    for layout, shape in (("fixed", L), ("ragged", np.arange(count + 1) * L)):
        st, e, o = call_reads(layout, False, False, s, shape, k, 0, pos, queries, query, end)
        gs, gd = o.read()
        assert st == 0, (st, e.index)
        live = np.array([False, False, False, False, False, True, False])
        assert (gs[~live] == 0xFFFFFFFF).all() and (gd[~live] == 0xFF).all() and gs[live][0] <= 12 and gd[live][0] <= k
    ref = np.full(100, ord("N"), dtype=np.uint8)
    st, e, o = call_ref(False, False, ref, k, queries, [2, 0xFFFFFFFF, 0, 0xA5A5A5A5], [10, 10, 101, 0xA5A5A5A5A5A5A5A5])
    gs, gd = o.read()
    assert st == 0 and (gs == so.FILL64).all() and (gd == 0xFF).all()
    # k == 0 and no queries: every item is skipped, no data pointer is looked at
    lib = _L().load()
    for k0, nq in ((0, 2), (8, 0)):
        o = Out(3)
        q = np.zeros(3, dtype=np.uint32)
        st, e = _raw(lib.bitnuc_reads_edist_start, None, None, 30, 3, k0, 0, 0, _p(queries) if nq else None, nq, _p(q), _p(q), *o.ptrs())
        gs, gd = o.read()
        assert st == 0 and (gs == 0xFFFFFFFF).all() and (gd == 0xFF).all()
    # dist may be NULL
    st, e, o = call_reads("fixed", False, False, _ascii(rng.integers(0, 4, size=60)), 30, k, 0, 0, queries, [0, 1], [20, 30], with_dist=False)
    assert st == 0 and (o.read(False)[0] <= 30).all()


def test_argument_checks_in_their_order():
    L = _L()
    lib = L.load()
    k, count, rl = 8, 3, 30
    s = _ascii(np.zeros(count * rl, dtype=np.int64))
    off = np.arange(count + 1, dtype=np.uint64) * rl
    queries = np.array([0, 1], dtype=np.uint64)
    qi = np.zeros(count, dtype=np.uint32)
    en = np.full(count, 10, dtype=np.uint32)
    big = L.MAX_QUERIES + 1 if hasattr(L, "MAX_QUERIES") else 65537

    def fixed(o, data=s, read_len=rl, n=count, kk=k, anchor=0, q=queries, nq=2, query=qi, end=en, start="o"):
        sp, dp = o.ptrs()
        return _raw(lib.bitnuc_reads_edist_start, None, _p(data) if data is not None else None, read_len, n, kk, anchor, 0, _p(q) if q is not None else None, nq,
                    _p(query) if query is not None else None, _p(end) if end is not None else None, sp if start == "o" else start, dp)

    def expect(res, status, value=None):
        st, e = res
        assert st == status and e.status == status, (st, status)
        if value is not None:
            assert e.value == value, (e.value, value)

    o = Out(count)
    # each check fires although every later one would fire too
    expect(fixed(o, kk=33, read_len=2**32, nq=big, anchor=7, query=None), L.SEQUENCE_TOO_LONG, 33)
    expect(fixed(o, read_len=2**32 - 1, nq=big, anchor=7, query=None), L.UNSUPPORTED, 2**32 - 1)
    expect(fixed(o, nq=big, anchor=7, query=None), L.UNSUPPORTED, big)
    expect(fixed(o, anchor=7, query=None), L.UNSUPPORTED, 7)
    expect(fixed(o, n=0, query=None, data=None), L.OK)
    expect(fixed(o, query=None, data=None), L.UNSUPPORTED)
    expect(fixed(o, end=None, data=None), L.UNSUPPORTED)
    expect(fixed(o, start=None, data=None), L.UNSUPPORTED)
    expect(fixed(o, start=C.c_void_p(o.s.ctypes.data + 4 * GUARD + 2), data=None), L.UNSUPPORTED)
    expect(fixed(o, q=None, data=None), L.UNSUPPORTED)
    odd = np.zeros(4, dtype=np.uint64)
    st, e = _raw(lib.bitnuc_reads_edist_start, None, _p(s), rl, count, k, 0, 0, C.c_void_p(odd.ctypes.data + 4), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    st, e = _raw(lib.bitnuc_reads_pattern_edist_start, None, _p(s), rl, count, k, 0, 0, C.c_void_p(odd.ctypes.data + 2), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    expect(fixed(o, data=None), L.UNSUPPORTED)
    assert o.untouched()
    # packed words must be 8-byte aligned; the ragged forms: a NULL or misaligned table, then the tables' validation, then the data pointer
    w = ro.pack_reads(s, rl, count)
    st, e = _raw(lib.bitnuc_reads_edist_start_packed, None, C.c_void_p(w.ctypes.data + 4), rl, count, k, 0, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    st, e = _raw(lib.bitnuc_reads_edist_start_batch, None, None, None, count, k, 0, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    badoff = off.copy()
    badoff[2] = badoff[1] - 1
    st, e = _raw(lib.bitnuc_reads_edist_start_batch, None, None, _p(badoff), count, k, 0, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.INVALID_RANGE
    st, e = _raw(lib.bitnuc_reads_edist_start_batch, None, None, _p(off), count, k, 0, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    woff = rb.word_offsets_of(off)
    st, e = _raw(lib.bitnuc_reads_edist_start_batch_packed, None, _p(w), None, _p(off), count, k, 0, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED
    st, e = _raw(lib.bitnuc_reads_edist_start_batch_packed, None, _p(w), _p(woff), _p(off), count, k, 9, 0, _p(queries), 2, _p(qi), _p(en), *o.ptrs())
    assert st == L.UNSUPPORTED and e.value == 9
    assert o.untouched()
    # along a reference
    ends = np.array([5, 6], dtype=np.uint64)
    r = Out(2, wide=True)

    def ref(fn=lib.bitnuc_ref_edist_start, head=(_p(s), s.size), kk=k, q=_p(queries), nq=2, qidx=None, end=_p(ends), m=2, start="r"):
        sp, dp = r.ptrs()
        return _raw(fn, None, *head, kk, q, nq, qidx, end, m, sp if start == "r" else start, dp)

    expect(ref(kk=33, nq=big, end=None), L.SEQUENCE_TOO_LONG, 33)
    expect(ref(fn=lib.bitnuc_ref_edist_start_packed, head=(_p(w), 0, 40), nq=big, end=None), L.INVALID_LENGTH, 40)
    expect(ref(m=0, nq=big, end=None), L.OK)
    expect(ref(nq=big, end=None), L.UNSUPPORTED, big)
    expect(ref(end=None), L.UNSUPPORTED)
    expect(ref(start=None), L.UNSUPPORTED)
    expect(ref(end=C.c_void_p(ends.ctypes.data + 4)), L.UNSUPPORTED)
    expect(ref(qidx=C.c_void_p(qi.ctypes.data + 2)), L.UNSUPPORTED)
    expect(ref(q=None), L.UNSUPPORTED)
    expect(ref(head=(None, s.size)), L.UNSUPPORTED)
    expect(ref(fn=lib.bitnuc_ref_edist_start_packed, head=(C.c_void_p(w.ctypes.data + 4), w.size - 1, 32)), L.UNSUPPORTED)
    assert r.untouched()
    expect(ref(), L.OK)


def test_all_256_byte_values_at_every_walked_position_and_beside_the_walked_range():
    k = 3  # the window: the five bytes in front of the end
    valid = set(b"ACGTacgt")
    queries = np.array([ro.word_of([0, 1, 2])], dtype=np.uint64)
    base = np.frombuffer(b"GATTACAGATTACAGG", dtype=np.uint8)
    e = 11
    paths = {
        "fixed": lambda t: call_reads("fixed", False, False, t, 16, k, 0, 0, queries, [0], [e]),
        "ragged": lambda t: call_reads("ragged", False, False, t, [0, 16], k, 0, 0, queries, [0], [e]),
        "ragged, second read": lambda t: call_reads("ragged", False, False, np.concatenate([base, t]), [0, 16, 32], k, 0, 0, queries, [9, 0], [0, e]),
        "reference": lambda t: call_ref(False, False, t, k, queries, None, [e]),
    }
    for name, run in paths.items():
        shift = 16 if name == "ragged, second read" else 0
        st, err, o = run(base.copy())
        assert st == 0
        clean = o.read()
        for at in range(e - 5 - 1, e + 1):  # the byte in front of the window, its five bytes, the byte behind it
            for b in range(256):
                t = base.copy()
                t[at] = b
                st, err, o = run(t)
                if e - 5 <= at < e and b not in valid:
                    assert st == 1 and err.index == at + shift and err.byte == b and o.untouched(), (name, at, b, st)
                else:
                    assert st == 0, (name, at, b)
                    got = o.read()
                    if not (e - 5 <= at < e) or (b & 0xDF) == (base[at] & 0xDF):
                        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]), (name, at, b)
    # the first invalid walked byte in buffer order, over all items
    t = np.concatenate([base, base, base]).copy()
    t[16 + 8] = ord("N")
    t[32 + 7] = ord("n")
    st, err, o = call_reads("fixed", False, False, t, 16, k, 0, 0, queries, [0, 0, 0], [e, e, e])
    assert st == 1 and err.index == 24 and err.byte == ord("N") and o.untouched()
    st, err, o = call_ref(False, False, t, k, queries, None, [32 + e, 16 + e, e])  # items in any order: the smallest index
    assert st == 1 and err.index == 24 and o.untouched()


@pytest.mark.parametrize("k", [2, 16, 31])
def test_every_forward_host_form_followed_by_the_start_form(k):
    free = _free()
    rng = np.random.default_rng(0x1DE7 + k)
    Q = 3
    queries = np.array([ro.word_of(rng.permutation(np.arange(k) % 4)) for _ in range(Q)], dtype=np.uint64)
    pats = rp.singletons(queries, k)
    count = 60
    seen = 0
    # fixed-length and ragged batches of planted reads
    for ragged in (False, True):
        if ragged:
            s, off = _planted(rng, k, count, queries)
        else:
            L = 2 * k + 30
            off = np.arange(count + 1, dtype=np.uint64) * L
            s = _ascii(rng.integers(0, 4, size=count * L))
            for r in range(count):
                c = [int(x) for x in ro.query_codes(queries[r % Q], k)]
                if r % 3 == 0 and k >= 3:
                    del c[k // 2]
                at = r * L + int(rng.integers(0, L - len(c) + 1))
                s[at:at + len(c)] = _ascii(c)
        codes = ro.codes_of(s)
        texts = [codes[int(off[r]):int(off[r + 1])] for r in range(count)]
        for pattern in (False, True):
            qs = pats if pattern else queries
            pre = "reads_pattern_edist_" if pattern else "reads_edist_"
            for packed in (False, True):
                forms = []
                if ragged:
                    data = (rb.pack_batch(s, off, seed=k), rb.word_offsets_of(off), off) if packed else (s, off)
                    sfx = "_batch_packed" if packed else "_batch"
                    forms.append((getattr(free, pre + "best" + sfx), data + (k, qs), {}, (0, 0)))
                    for anchor, lo, hi in (("start", 2, 2 + min(20, 63 - k)), ("end", 0, min(20, 63 - k))):
                        forms.append((getattr(free, pre + "anchored" + sfx), data + (k, qs), dict(pos_lo=lo, pos_hi=hi, anchor=anchor),
                                      (1, hi) if anchor == "end" else (0, lo)))
                else:
                    L = int(off[1])
                    data = (ro.pack_reads(s, L, count), L, count) if packed else (s, L)
                    sfx = "_packed" if packed else ""
                    forms.append((getattr(free, pre + "best" + sfx), data + (k, qs), {}, (0, 0)))
                    forms.append((getattr(free, pre + "anchored" + sfx), data + (k, qs), dict(pos_lo=3, pos_hi=3 + min(25, 63 - k)), (0, 3)))
                for fn, args, kw, (anchor_end, pos) in forms:
                    res = fn(*args, with_start=True, **kw)
                    assert len(res) == 8 and fn(*args, **kw)[0].shape == res[0].shape
                    seen += 1
                    floors = [so.floor_of(len(t), k, anchor_end, pos) for t in texts]
                    for j in (0, 1):
                        fq, fe, fd, start = res[3 * j], res[3 * j + 1], res[3 * j + 2], res[6 + j]
                        ws, wd = so.starts(texts, floors, so.masks_of(queries, k), k, fq, fe)
                        assert np.array_equal(start, ws.astype(np.uint32))
                        live = fq != 0xFFFFFFFF
                        assert live.any() and np.array_equal(wd[live], fd[live]) and (start[live] <= fe[live]).all()
                        assert (start[~live] == 0xFFFFFFFF).all()
    assert seen == 16 + 4  # the 16 forward per-read host forms, the four ragged anchored ones under both anchors
    # along a reference: best, and hits with and without a cap
    n = 3000
    ref = _ascii(rng.integers(0, 4, size=n))
    for i, at in enumerate((100, 900, 2000)):
        c = [int(x) for x in ro.query_codes(queries[i], k)]
        if i == 1 and k >= 3:
            del c[k // 2]
        ref[at:at + len(c)] = _ascii(c)
    rc = ro.codes_of(ref)
    w = ro.pack_reads(ref, n, 1)
    seen = 0
    for pattern in (False, True):
        qs = pats if pattern else queries
        pre = "kmer_pattern_edist_" if pattern else "kmer_edist_"
        for packed in (False, True):
            head = (w, n) if packed else (ref,)
            sfx = "_packed" if packed else ""
            end, dist, start = getattr(free, pre + "best" + sfx)(*head, k, qs, with_start=True)
            seen += 1
            ws, wd = so.starts([rc] * Q, [0] * Q, so.masks_of(queries, k), k, np.arange(Q), end, fill=so.FILL64)
            assert np.array_equal(start, ws) and np.array_equal(dist, wd) and (start <= end).all()
            one = qs[1] if pattern else int(queries[1])
            ends, hd, start = getattr(free, pre + "hits" + sfx)(*head, k, one, 1, with_dist=True, with_start=True)
            seen += 1
            assert ends.size >= 1
            ws, wd = so.starts([rc] * ends.size, [0] * ends.size, so.masks_of(queries[1:2], k), k, np.zeros(ends.size, dtype=np.int64), ends, fill=so.FILL64)
            assert np.array_equal(start, ws) and np.array_equal(hd, wd) and (start <= ends).all()
            # with a cap below the number of hits: the raw call leaves end[cap ...) unwritten; items there are whatever the caller put
            lib = _L().load()
            cap = max(1, ends.size - 1)
            e_cap = np.full(ends.size, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            total = C.c_uint64(0)
            q1 = rp.as_patterns(qs)[1:2] if pattern else None
            name = "bitnuc_kmer_" + ("pattern_" if pattern else "") + "edist_hits" + sfx
            hhead = (_p(w), w.size, n) if packed else (_p(ref), n)
            st, err = _raw(getattr(lib, name), None, *hhead, k, _p(q1) if pattern else C.c_uint64(one), 1, _p(e_cap), None, cap, C.byref(total))
            assert st == 0 and total.value == ends.size
            seen += 1
            st, err, o = call_ref(packed, pattern, ref, k, qs[1:2], None, e_cap)
            gs, gd = o.read()
            assert st == 0 and np.array_equal(gs[:cap], ws[:cap]) and np.array_equal(gd[:cap], wd[:cap])
            assert (gs[cap:] == so.FILL64).all() and (gd[cap:] == 0xFF).all()
    assert seen == 12
