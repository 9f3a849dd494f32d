"""CPU tests (no GPU) of the alphabet on the library's HOST forms below the cutoff -- bitnuc_encode (csrc/host_word.h), bitnuc_kmer_hdist_hits
(csrc/scan_hits_host.h) and bitnuc_kmer_hdist_count_multi (csrc/scan_multi_host.h) through a NULL context: all 256 byte values at every position
of sequences of 7 .. 34 bases (every i % 8, both sides of the 8- and 32-base steps of the SWAR code).  An invalid byte comes back as
InvalidBase(byte, index) exactly as the oracle reports it, a later invalid byte of the other class never wins, the hits and counts outputs are left
as they were (their headers' "nothing written" / "counts untouched"), and the eight valid values give the oracle's result in either case.

The second half (HostForm, _sweep) runs the same sweep over the host forms of the search entry points that came later, one test per host header:
along a reference on the same 7 .. 34 bases, per read on three to five reads of 7 .. 40 bases with k smaller than, equal to and larger than a read.
There the bytes an entry point OWNS are written down from its header's validation paragraph (all of them, the span bytes [pos_lo, hi_eff + k), the reads
of at least k bases, none without a window): an owned byte is refused for each of the 248 invalid values, with its absolute index and every output
left as it was; every other byte is ignored for all 256 values and the call gives the family oracle's result for the unpolluted input."""
import ctypes as C
import zlib

import numpy as np
import pytest

import alphabet as ab

LENGTHS = (7, 8, 9, 31, 32, 33, 34)
QUERIES = np.array([0x1B1B1B1B1B1B1B1B, 0, 0xE4E4E4E4E4E4E4E4, 0x3FFFFFFFFFFFFFFF, 0x123456789ABCDEF0], dtype=np.uint64)
TAUS = np.array([1, 2, 0, 3, 2**32 - 1], dtype=np.uint32)


@pytest.fixture(scope="module")
def lib():
    from bitnuc_amd import _lib as L
    from bitnuc_amd import build
    build.ensure_built()
    return L, L.load()


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _cases():
    """(n, position, byte, second position or None): every byte value at every position of every length; a second invalid byte of the other class
    later in the sequence whenever there is room"""
    for n in LENGTHS:
        for pos in range(n):
            for b in range(256):
                later = pos + 1 + (b % (n - pos - 1)) if pos + 1 < n else None
                yield n, pos, b, later


def _expect(oracle, call):
    try:
        return None, call()
    except oracle.OracleError as e:
        return e, None


def test_encode_all_values_at_every_position(lib, oracle):
    L, so = lib
    rng = np.random.default_rng(0xA1FA)
    good = {n: ab.bases(rng, n) for n in LENGTHS}
    fails = []
    for n, pos, b, later in _cases():
        s = good[n].copy()
        s[pos] = b
        if later is not None and b not in ab.VALID:
            s[later] = ab.other_class(b, pos)
        out = np.full((n + 31) // 32 + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        nw, err = C.c_size_t(99), L.BitnucErr()
        st = so.bitnuc_encode(None, _p(s), n, _p(out), C.byref(nw), C.byref(err))
        e, want = _expect(oracle, lambda: oracle.encode(s))
        tag = f"encode n={n} {ab.describe(b)} at {pos}"
        if e is not None:
            if (st, int(err.byte), int(err.index)) != (L.INVALID_BASE, b, pos) or (e.byte, e.index) != (b, pos):
                fails.append(tag + f": status {st} byte {int(err.byte)} index {int(err.index)}, oracle byte {e.byte} index {e.index}")
            elif nw.value != e.words.size or not np.array_equal(out[:nw.value], e.words):
                fails.append(tag + ": the words before the failing chunk differ from the oracle's")
        elif st != L.OK or nw.value != want.size or not np.array_equal(out[:want.size], want):
            fails.append(tag + f": status {st}, words differ from the oracle's")
        if not (out[(n + 31) // 32:] == 0xA5A5A5A5A5A5A5A5).all():
            fails.append(tag + ": wrote past ceil(n / 32) words")
    assert not fails, "\n".join(fails[:20]) + f"\n({len(fails)} failing cases)"


def test_hits_all_values_at_every_position(lib, oracle):
    L, so = lib
    rng = np.random.default_rng(0xA1FB)
    good = {n: ab.bases(rng, n) for n in LENGTHS}
    fails = []
    for n, pos, b, later in _cases():
        s = good[n].copy()
        s[pos] = b
        if later is not None and b not in ab.VALID:
            s[later] = ab.other_class(b, pos)
        for k in (5, min(n, 31)):
            query, tau, cap = int(QUERIES[(pos + k) % QUERIES.size]), k - 1 - (pos % 2), n
            hp = np.full(cap + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            hd = np.full(cap + 2, 0xEE, dtype=np.uint8)
            nh, err = C.c_uint64(0x7777), L.BitnucErr()
            st = so.bitnuc_kmer_hdist_hits(None, _p(s), n, k, C.c_uint64(query), tau, _p(hp), _p(hd), cap, C.byref(nh), C.byref(err))
            e, d = _expect(oracle, lambda: oracle.kmer_hdist_scan(s, k, query))
            tag = f"hits n={n} k={k} {ab.describe(b)} at {pos}"
            if e is not None:
                if (st, int(err.byte), int(err.index)) != (L.INVALID_BASE, b, pos) or (e.byte, e.index) != (b, pos):
                    fails.append(tag + f": status {st} byte {int(err.byte)} index {int(err.index)}, oracle byte {e.byte} index {e.index}")
                if nh.value != 0x7777 or not (hp == 0xA5A5A5A5A5A5A5A5).all() or not (hd == 0xEE).all():
                    fails.append(tag + ": an output was written although the call failed")
                continue
            want = np.flatnonzero(d <= tau)
            if st != L.OK or nh.value != want.size or not np.array_equal(hp[:want.size], want) or not np.array_equal(hd[:want.size], d[want]):
                fails.append(tag + f": status {st} n_hits {nh.value}, oracle {want.size}, or the hits differ")
            if not (hp[want.size:] == 0xA5A5A5A5A5A5A5A5).all() or not (hd[want.size:] == 0xEE).all():
                fails.append(tag + ": wrote past the hits")
    assert not fails, "\n".join(fails[:20]) + f"\n({len(fails)} failing cases)"


def test_count_multi_all_values_at_every_position(lib, oracle):
    L, so = lib
    rng = np.random.default_rng(0xA1FC)
    good = {n: ab.bases(rng, n) for n in LENGTHS}
    nq = QUERIES.size
    fails = []
    for n, pos, b, later in _cases():
        s = good[n].copy()
        s[pos] = b
        if later is not None and b not in ab.VALID:
            s[later] = ab.other_class(b, pos)
        for k in (5, min(n, 31)):
            taus = np.minimum(TAUS, np.uint32(max(k - 1, 0))).astype(np.uint32) if pos % 2 else TAUS
            counts = np.full(nq + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            err = L.BitnucErr()
            st = so.bitnuc_kmer_hdist_count_multi(None, _p(s), n, k, _p(QUERIES), _p(taus), nq, _p(counts), C.byref(err))
            e, ds = _expect(oracle, lambda: [oracle.kmer_hdist_scan(s, k, int(q)) for q in QUERIES])
            tag = f"count_multi n={n} k={k} {ab.describe(b)} at {pos}"
            if e is not None:
                if (st, int(err.byte), int(err.index)) != (L.INVALID_BASE, b, pos) or (e.byte, e.index) != (b, pos):
                    fails.append(tag + f": status {st} byte {int(err.byte)} index {int(err.index)}, oracle byte {e.byte} index {e.index}")
                if not (counts == 0xA5A5A5A5A5A5A5A5).all():
                    fails.append(tag + ": counts were written although the call failed")
                continue
            want = np.array([int((d <= int(t)).sum()) for d, t in zip(ds, taus)], dtype=np.uint64)
            if st != L.OK or not np.array_equal(counts[:nq], want):
                fails.append(tag + f": status {st} counts {counts[:nq].tolist()}, oracle {want.tolist()}")
            if not (counts[nq:] == 0xA5A5A5A5A5A5A5A5).all():
                fails.append(tag + ": wrote past counts[n_queries)")
    assert not fails, "\n".join(fails[:20]) + f"\n({len(fails)} failing cases)"


def test_host_forms_ignore_case(lib, oracle):
    L, so = lib
    rng = np.random.default_rng(0xA1FD)
    for n in LENGTHS + (200, 1057):
        s = ab.bases(rng, n)
        k, query, tau = min(n, 21), int(QUERIES[n % QUERIES.size]), 12
        d = oracle.kmer_hdist_scan(ab.recase(s, "upper"), k, query)
        want_hits = np.flatnonzero(d <= tau)
        want_words = oracle.encode(ab.recase(s, "upper"))
        want_counts = np.array([int((oracle.kmer_hdist_scan(s, k, int(q)) <= int(t)).sum()) for q, t in zip(QUERIES, TAUS)], dtype=np.uint64)
        for case in ("upper", "lower", "mixed"):
            t = ab.recase(s, case, n)
            out, nw, err = np.zeros((n + 31) // 32, dtype=np.uint64), C.c_size_t(0), L.BitnucErr()
            assert so.bitnuc_encode(None, _p(t), n, _p(out), C.byref(nw), C.byref(err)) == L.OK
            assert np.array_equal(out, want_words) and np.array_equal(oracle.encode(t), want_words), (n, case)
            hp, hd, nh = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8), C.c_uint64(0)
            assert so.bitnuc_kmer_hdist_hits(None, _p(t), n, k, C.c_uint64(query), tau, _p(hp), _p(hd), n, C.byref(nh), C.byref(err)) == L.OK
            assert nh.value == want_hits.size and np.array_equal(hp[:nh.value], want_hits) and np.array_equal(hd[:nh.value], d[want_hits]), (n, case)
            counts = np.zeros(QUERIES.size, dtype=np.uint64)
            assert so.bitnuc_kmer_hdist_count_multi(None, _p(t), n, k, _p(QUERIES), _p(TAUS), QUERIES.size, _p(counts), C.byref(err)) == L.OK
            assert np.array_equal(counts, want_counts), (n, case)


# ---- the host forms of the later search entry points -------------------------------------------------------------------------------------
SIZE_MAX = 2**64 - 1
GUARDS = {np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5, np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint8): 0xEE}
U32x2_U8 = (np.uint32, np.uint32, np.uint8)


class HostForm:
    """One call shape of a host form.  good: the valid input; owned: the positions the header says are validated (ascending); outs: [(dtype, elements)]
    the call must write exactly; call(s, out pointers, err) -> status; want(s) -> the oracle's outputs for a valid s."""

    def __init__(self, name, good, owned, outs, call, want):
        self.name, self.good, self.owned, self.outs, self.call, self.want = name, good, np.asarray(owned, dtype=np.int64), outs, call, want


def _sweep(L, forms):
    """Every output of a form lies in ONE byte buffer, each behind and in front of guard elements, so a call is checked with one comparison: against
    the buffer as it was (an error: nothing written) or with the oracle's values written into it (exactly [0, n) of each output, nothing behind)."""
    fails = []
    for F in forms:
        at, size = [], 0
        for dt, n in F.outs:
            at.append(size)
            size += -(-((n + 2) * np.dtype(dt).itemsize) // 8) * 8  # two guard elements behind each output, 8-byte aligned starts
        untouched = np.zeros(size, dtype=np.uint8)
        for (dt, n), a in zip(F.outs, at):
            untouched[a:a + (n + 2) * np.dtype(dt).itemsize] = np.full(n + 2, GUARDS[np.dtype(dt)], dtype=dt).view(np.uint8)
        buf = untouched.copy()
        ptrs = [C.c_void_p(buf.ctypes.data + a) for a in at]
        err = L.BitnucErr()

        def expected(outs):
            e = untouched.copy()
            for w, (dt, n), a in zip(outs, F.outs, at):
                w = np.ascontiguousarray(np.asarray(w).reshape(-1).astype(dt))
                assert w.size == n, (F.name, w.size, n)
                e[a:a + w.nbytes] = w.view(np.uint8)
            return e

        def check(tag, s, exp):
            buf[:] = untouched
            st = F.call(s, ptrs, err)
            if st != L.OK:
                fails.append(tag() + f": status {st} byte {int(err.byte)} index {int(err.index)}")
            elif not np.array_equal(buf, exp):
                fails.append(tag() + f": the outputs differ from the oracle's, or something was written behind them (byte {int(np.flatnonzero(buf != exp)[0])} of the buffer)")
        is_owned = np.zeros(F.good.size, dtype=bool)
        is_owned[F.owned] = True
        base = expected(F.want(F.good))
        for case in ("upper", "lower"):
            s = ab.recase(F.good, case)
            s[~is_owned] = F.good[~is_owned]
            check(lambda: f"{F.name} {case} case", s, base)
        s = F.good.copy()
        for pos in range(F.good.size):
            later = F.owned[F.owned > pos]
            by_code = {((int(F.good[pos]) >> 1) ^ (int(F.good[pos]) >> 2)) & 3: base}
            for b in range(256):
                tag = lambda: f"{F.name} {ab.describe(b) if b not in ab.VALID else chr(b)} at {pos} ({'owned' if is_owned[pos] else 'not owned'})"  # noqa: E731
                s[pos] = b
                if is_owned[pos] and b not in ab.VALID:
                    second = int(later[b % later.size]) if later.size else None
                    if second is not None:
                        s[second] = ab.other_class(b, pos)
                    buf[:] = untouched
                    st = F.call(s, ptrs, err)
                    if (st, int(err.byte), int(err.index)) != (L.INVALID_BASE, b, pos):
                        fails.append(tag() + f": status {st} byte {int(err.byte)} index {int(err.index)}")
                    if not np.array_equal(buf, untouched):
                        fails.append(tag() + ": an output was written although the call failed")
                    if second is not None:
                        s[second] = F.good[second]
                elif not is_owned[pos]:
                    check(tag, s, base)
                else:  # one of the eight valid values: the oracle once per base (either case is the same base)
                    code = ((b >> 1) ^ (b >> 2)) & 3
                    if code not in by_code:
                        by_code[code] = expected(F.want(s))
                    check(tag, s, by_code[code])
            s[pos] = F.good[pos]
    assert not fails, "\n".join(fails[:20]) + f"\n({len(fails)} failing cases)"


def _ref_forms(name, make, ks=lambda n: (5, min(n, 31))):
    """along a reference: every byte of the n is validated when there is a window (k <= n)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for n in LENGTHS:
        for k in ks(n):
            good = ab.bases(rng, n)
            yield make(f"{name} n={n} k={k}", good, np.arange(n), n, k)


def test_kmer_hdist_best_all_values_at_every_position(lib, oracle):
    L, so = lib
    nq = QUERIES.size

    def make(name, good, owned, n, k):
        def want(s):
            d = [oracle.kmer_hdist_scan(s, k, int(q)) for q in QUERIES]
            return [np.array([int(np.argmin(x)) for x in d], dtype=np.uint64), np.array([int(x.min()) for x in d], dtype=np.uint8)]
        return HostForm(name, good, owned, [(np.uint64, nq), (np.uint8, nq)],
                        lambda s, o, err: so.bitnuc_kmer_hdist_best(None, _p(s), n, k, _p(QUERIES), nq, o[0], o[1], C.byref(err)), want)
    _sweep(L, _ref_forms("kmer_hdist_best", make))


def test_kmer_hdist_hist_all_values_at_every_position(lib, oracle):
    import hist_oracle as ho
    L, so = lib
    nq = QUERIES.size

    def make(name, good, owned, n, k):
        n_bins = 8 if n % 2 else 16
        return HostForm(name + f" n_bins={n_bins}", good, owned, [(np.uint64, nq * n_bins)],
                        lambda s, o, err: so.bitnuc_kmer_hdist_hist(None, _p(s), n, k, _p(QUERIES), nq, n_bins, o[0], C.byref(err)),
                        lambda s: [ho.hist(oracle, s, k, [int(q) for q in QUERIES], n_bins)])
    _sweep(L, _ref_forms("kmer_hdist_hist", make))


def test_kmer_pattern_hits_all_values_at_every_position(lib, oracle):
    import pattern_oracle as po
    L, so = lib

    def make(name, good, owned, n, k):
        pat = po.from_sets([{0, 1, 2, 3} if i % 4 == 1 else {(int(QUERIES[n % QUERIES.size]) >> (2 * i)) & 3} for i in range(k)])
        tau = k - 2

        def want(s):
            pos, dist, total = po.hits(po.pdist(po.codes_of_ascii(s), pat, k), tau, n)
            full = lambda a, dt: np.concatenate([a.astype(dt), np.full(n - a.size, GUARDS[np.dtype(dt)], dtype=dt)])  # noqa: E731
            return [full(pos, np.uint64), full(dist, np.uint8), np.array([total], dtype=np.uint64)]

        def call(s, o, err):
            return so.bitnuc_kmer_pattern_hits(None, _p(s), n, k, _p(pat), tau, o[0], o[1], n, C.cast(o[2], C.POINTER(C.c_uint64)), C.byref(err))
        return HostForm(name, good, owned, [(np.uint64, n), (np.uint8, n), (np.uint64, 1)], call, want)
    _sweep(L, _ref_forms("kmer_pattern_hits", make))


def test_kmer_edist_best_all_values_at_every_position(lib, oracle):
    import kmer_edist_oracle as ko
    import reads_best_oracle as ro
    L, so = lib
    q3 = np.ascontiguousarray(QUERIES[:3])

    def make(name, good, owned, n, k):
        return HostForm(name, good, owned, [(np.uint64, 3), (np.uint8, 3)],
                        lambda s, o, err: so.bitnuc_kmer_edist_best(None, _p(s), n, k, _p(q3), 3, o[0], o[1], C.byref(err)),
                        lambda s: list(ko.kmer_edist_best(ro.codes_of(s), k, ko.singletons(q3, k))))
    _sweep(L, _ref_forms("kmer_edist_best", make))


def test_kmer_edist_hits_all_values_at_every_position(lib, oracle):
    import kmer_edist_hits_oracle as kh
    import pattern_oracle as po
    import reads_best_oracle as ro
    L, so = lib

    def make(name, good, owned, n, k):
        query, tau = int(QUERIES[(n + k) % QUERIES.size]), k - 2

        def want(s):
            e, d = kh.hits(ro.codes_of(s), k, po.from_2bit(query, k), tau)
            full = lambda a, dt: np.concatenate([a.astype(dt), np.full(n - a.size, GUARDS[np.dtype(dt)], dtype=dt)])  # noqa: E731
            return [full(e, np.uint64), full(d, np.uint8), np.array([e.size], dtype=np.uint64)]

        def call(s, o, err):
            return so.bitnuc_kmer_edist_hits(None, _p(s), n, k, C.c_uint64(query), tau, o[0], o[1], n, C.cast(o[2], C.POINTER(C.c_uint64)), C.byref(err))
        return HostForm(name, good, owned, [(np.uint64, n), (np.uint8, n), (np.uint64, 1)], call, want)
    _sweep(L, _ref_forms("kmer_edist_hits", make))


# per read: (read_len, count, k) with k smaller than, equal to and larger than a read; the ragged batches hold an empty read and reads on both sides of k
FIXED_SHAPES = ((7, 5, 5), (7, 5, 7), (7, 5, 9), (40, 3, 16), (33, 4, 32), (9, 4, 4))
RAGGED_SHAPES = (((7, 0, 3, 12, 9), 5), ((7, 0, 3, 12, 9), 9), ((7, 0, 3, 12, 9), 13), ((40, 15, 16, 17), 16), ((33, 8, 32), 32))
ANCHORS = ((0, None), (2, 3), (1, 1))  # pos_lo, pos_hi (None: to the end of the read)
Q4 = np.ascontiguousarray(QUERIES[:4])


def _fixed_forms(name, make, anchors=(None,)):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for read_len, count, k in FIXED_SHAPES[:4 if anchors[0] else None]:  # (three anchors each: the first four shapes)
        for anchor in anchors:
            yield make(f"{name} read_len={read_len} count={count} k={k}" + (f" pos_lo={anchor[0]} pos_hi={anchor[1]}" if anchor else ""),
                       ab.bases(rng, read_len * count), read_len, count, k, anchor)


def _span_owned(read_len, count, k, anchor):
    """the header: only the span bytes [pos_lo, hi_eff + k) of each read, hi_eff = min(pos_hi, read_len - k); no window: nothing"""
    lo, hi = anchor
    if read_len < k:
        return np.zeros(0, dtype=np.int64)
    hi_eff = read_len - k if hi is None else min(hi, read_len - k)
    if lo > hi_eff:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([r * read_len + np.arange(lo, hi_eff + k) for r in range(count)])


def _six(count):
    return [(dt, count) for dt in U32x2_U8 * 2]


def test_reads_hdist_best_and_best2_all_values_at_every_position(lib, oracle):
    import reads_best2_oracle as r2
    import reads_best_oracle as ro
    L, so = lib

    def make(second):
        def m(name, good, read_len, count, k, _):
            owned = np.arange(good.size) if read_len >= k else []
            if second:
                return HostForm(name, good, owned, _six(count),
                                lambda s, o, err: so.bitnuc_reads_hdist_best2(None, _p(s), read_len, count, k, _p(Q4), 4, *o, C.byref(err)),
                                lambda s: list(r2.reads_best2(s, read_len, count, k, Q4)))
            return HostForm(name, good, owned, _six(count)[:3],
                            lambda s, o, err: so.bitnuc_reads_hdist_best(None, _p(s), read_len, count, k, _p(Q4), 4, *o, C.byref(err)),
                            lambda s: list(ro.reads_best(s, read_len, count, k, Q4)))
        return m
    _sweep(L, list(_fixed_forms("reads_hdist_best", make(False))) + list(_fixed_forms("reads_hdist_best2", make(True))))


def _ragged_forms(name, make, anchors=(None,)):
    import reads_batch_oracle as rb
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for lens, k in RAGGED_SHAPES:
        for anchor in anchors:
            offsets = rb.offsets_of(lens)
            yield make(f"{name} lengths={lens} k={k}" + (f" anchor={anchor}" if anchor else ""), ab.bases(rng, int(offsets[-1])), offsets, k, anchor)


def test_reads_hdist_best_batch_all_values_at_every_position(lib, oracle):
    """the header: every byte of seq[0 .. total_bases) is validated, whether or not its read is long enough to hold a window"""
    import reads_batch_oracle as rb
    L, so = lib

    def make(name, good, offsets, k, _):
        count = offsets.size - 1
        return HostForm(name, good, np.arange(good.size), _six(count)[:3],
                        lambda s, o, err: so.bitnuc_reads_hdist_best_batch(None, _p(s), _p(offsets), count, k, _p(Q4), 4, *o, C.byref(err)),
                        lambda s: list(rb.batch_best(s, offsets, k, Q4)))
    _sweep(L, _ragged_forms("reads_hdist_best_batch", make))


def test_reads_hdist_and_edist_anchored_all_values_at_every_position(lib, oracle):
    import reads_anchored_oracle as ra
    import reads_edist_oracle as eo
    L, so = lib

    def make(fn, orc):
        def m(name, good, read_len, count, k, anchor):
            lo, hi = anchor
            return HostForm(name, good, _span_owned(read_len, count, k, anchor), _six(count),
                            lambda s, o, err: fn(None, _p(s), read_len, count, k, lo, SIZE_MAX if hi is None else hi, _p(Q4), 4, *o, C.byref(err)),
                            lambda s: list(orc(s, read_len, count, k, Q4, lo, hi)))
        return m
    _sweep(L, list(_fixed_forms("reads_hdist_anchored", make(so.bitnuc_reads_hdist_anchored, ra.reads_anchored), ANCHORS))
           + list(_fixed_forms("reads_edist_anchored", make(so.bitnuc_reads_edist_anchored, eo.reads_edist), ANCHORS)))


RAGGED_ANCHORS = (("start", 0, 8), ("start", 2, 3), ("end", 0, 8), ("end", 1, 1))


def test_reads_hdist_and_edist_anchored_batch_all_values_at_every_position(lib, oracle):
    """the header: of a read with n_r admissible offsets only the n_r + k - 1 span bytes; a read without a window is not validated at all"""
    import reads_anchored_batch_oracle as rab
    import reads_edist_batch_oracle as eb
    L, so = lib

    def make(fn, orc):
        def m(name, good, offsets, k, anchor):
            kind, lo, hi = anchor
            count = offsets.size - 1
            owned = np.flatnonzero(rab.span_bytes(offsets, k, kind, lo, hi))
            return HostForm(name, good, owned, _six(count),
                            lambda s, o, err: fn(None, _p(s), _p(offsets), count, k, int(kind == "end"), lo, hi, _p(Q4), 4, *o, C.byref(err)),
                            lambda s: list(orc(s, offsets, k, Q4, kind, lo, hi)))
        return m
    _sweep(L, list(_ragged_forms("reads_hdist_anchored_batch", make(so.bitnuc_reads_hdist_anchored_batch, rab.reads_anchored_batch), RAGGED_ANCHORS))
           + list(_ragged_forms("reads_edist_anchored_batch", make(so.bitnuc_reads_edist_anchored_batch, eb.reads_edist_batch), RAGGED_ANCHORS)))


def test_reads_edist_best_and_best_batch_all_values_at_every_position(lib, oracle):
    """the header: every byte of every read (read_len >= k); ragged: a read shorter than k is neither read nor validated"""
    import reads_edist_best_oracle as ebo
    L, so = lib

    def fixed(name, good, read_len, count, k, _):
        return HostForm(name, good, np.arange(good.size) if read_len >= k else [], _six(count),
                        lambda s, o, err: so.bitnuc_reads_edist_best(None, _p(s), read_len, count, k, _p(Q4), 4, *o, C.byref(err)),
                        lambda s: list(ebo.reads_edist_best(s, read_len, count, k, Q4)))

    def ragged(name, good, offsets, k, _):
        count = offsets.size - 1
        off = offsets.astype(np.int64)
        owned = np.concatenate([np.arange(off[r], off[r + 1]) for r in range(count) if off[r + 1] - off[r] >= k] + [np.zeros(0, dtype=np.int64)])
        return HostForm(name, good, owned, _six(count),
                        lambda s, o, err: so.bitnuc_reads_edist_best_batch(None, _p(s), _p(offsets), count, k, _p(Q4), 4, *o, C.byref(err)),
                        lambda s: list(ebo.reads_edist_best_batch(s, offsets, k, Q4)))
    _sweep(L, list(_fixed_forms("reads_edist_best", fixed)) + list(_ragged_forms("reads_edist_best_batch", ragged)))
