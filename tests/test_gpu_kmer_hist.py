"""GPU tests of the mismatch histogram per query (bitnuc_kmer_hdist_hist[_packed]_async, bitnuc_kmer_pattern_hist[_packed]_async and the host forms
on a live context; scan_hist_device.h): hist[q, d] = the windows at distance exactly d < n_bins, against np.bincount over the oracle's scan
(tests/hist_oracle.py: references with planted copies of the queries, the expected value held to `assert_rich` before the library is called) --
every k, sizes around the round / trip / halo / tail boundaries, n_bins around the tier of eight bins, query counts around the query block of 16, ASCII
at byte offsets +0 / +1 / +7 / +15 and packed words at both alignments; windows planted at the edges of the bins at every place a window can be
computed at; closed-form references that saturate an 8-bit field unless the flush is right; the identities with count_multi and best on the device;
guards of 0x5A around every output; limits and argument errors; invalid bytes; a hipGraph replay; a mixed queue with one sync; patterns; the host
forms above the cutoff; more than 2^32 windows in one bin; a seeded fuzz."""
import numpy as np
import pytest

import hist_oracle as ho
import kmer_wrap_plan as kw
import pattern_oracle as po

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1055, 1056, 1057, 4095, 4127, 4128, 4129, 10**6 + 7)
BINS = (1, 7, 8, 9, 16)
QS = (1, 16, 17)
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
LUT = ho.LUT


def _queries(rng, nq, k):
    """random queries with junk above 2k"""
    q = rng.integers(0, 2**62, size=nq, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1)
    if k < 32:
        q |= rng.integers(0, 2**62, size=nq, dtype=np.uint64) << np.uint64(2 * k)
    return q


def _pack(s):
    """the packed words of an ASCII sequence (junk above 2n in the last word)"""
    return po.pack_codes(po.codes_of_ascii(s), junk=0xDEADBEEFCAFEF00D)


def _dev_queries(queries):
    import torch
    return torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _dev_patterns(patterns):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(patterns, dtype=np.uint32)).view(np.int32).copy()).to("cuda:0")


def _output(nq, n_bins):
    """(buffer, pointer to the histogram): GUARD cells of 0x5A... before and after hist[0 .. nq * n_bins)"""
    import torch
    buf = torch.full((GUARD + nq * n_bins + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    return buf, buf.data_ptr() + 8 * GUARD


def _read(ctx, buf, nq, n_bins):
    ctx.sync()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:GUARD] == np.uint64(FILL)).all() and (h[GUARD + nq * n_bins:] == np.uint64(FILL)).all(), "hist written outside [0, n_queries * n_bins)"
    return h[GUARD:GUARD + nq * n_bins].reshape(nq, n_bins).copy()


def _raw(ctx, name, *args):
    """(status, err) of a raw call on the context's handle: Unsupported's err.value does not travel in the Python exception"""
    import ctypes as C
    from bitnuc_amd import _lib as L
    from bitnuc_amd.api import _dev_ptr
    err = L.BitnucErr()
    st = getattr(ctx._lib, name)(ctx._h, *[_dev_ptr(a) if i in _pointer_positions(len(args)) else a for i, a in enumerate(args)], C.byref(err))
    return st, err


def _pointer_positions(nargs):
    """the positions of the pointer arguments after ctx: the reference, the queries and the histogram"""
    return (0, nargs - 4, nargs - 1)


def _ascii_dev(s, off):
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    return t, t.data_ptr() + off


def _words_dev(w, off):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    return t, t.data_ptr() + 8 * off


def _both(ctx, s, k, queries, n_bins, off, woff, patterns=False):
    """(hist of the ASCII form, hist of the packed form), guards checked"""
    import torch
    n, nq = s.size, len(queries)
    t, ptr = _ascii_dev(s, off)
    w = _pack(s)
    tw, wptr = _words_dev(w, woff)
    assert wptr % 16 == 8 * woff
    dq = _dev_patterns(queries) if patterns else _dev_queries(queries)
    b1, h1 = _output(nq, n_bins)
    b2, h2 = _output(nq, n_bins)
    torch.cuda.synchronize()
    if patterns:
        ctx.kmer_pattern_hist_async(ptr, n, k, dq, nq, n_bins, h1)
        ctx.kmer_pattern_hist_packed_async(wptr, w.size, n, k, dq, nq, n_bins, h2)
    else:
        ctx.kmer_hdist_hist_async(ptr, n, k, dq, nq, n_bins, h1)
        ctx.kmer_hdist_hist_packed_async(wptr, w.size, n, k, dq, nq, n_bins, h2)
    got = _read(ctx, b1, nq, n_bins), _read(ctx, b2, nq, n_bins)
    del t, tw
    return got


# ---- 1. every k, size, n_bins, query count and offset ---------------------------------------------------------------------------------
def _case_1(k, si):
    """the rotation: every (size, n_bins), (size, Q), (size, offset) and (size, word parity) meets over the 32 k"""
    n = SIZES[si]
    return n, BINS[(si + k) % len(BINS)], QS[(si + k // 5) % len(QS)], (0, 1, 7, 15)[(si + k) % 4], (si + k // 4) % 2


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_size_bins_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(9100 + k)
    for si in range(len(SIZES)):
        n, n_bins, nq, off, woff = _case_1(k, si)
        queries = _queries(rng, nq, k)
        s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
        want = ho.hist(oracle, s, k, queries, n_bins)
        if ho.roomy(n, k, n_bins):
            ho.assert_rich(want, k, n_bins)
        a, p = _both(ctx, s, k, queries, n_bins, off, woff)
        assert np.array_equal(a, p), (n, n_bins, nq)
        assert np.array_equal(a, want), (n, n_bins, nq, np.argwhere(a != want)[:5])


# ---- 2. the edges of the bins at every place a window can be computed at ------------------------------------------------------------------
K_EDGE = 32
N_EDGE = 9 + 11 * 1024 + 32 + 200
# ASCII at byte offset +7: the rounds start at window 9; eleven rounds = two trips of four and a partial one of three (one trip per wave), the tail
# at 9 + 11 * 1024 = 11273.  A window's place in a round: 32 lane + 8 (register / 4) + 4 (lane / 32) + register % 4.
PLACES = {"head": (3,), "round 0": (9 + 100,), "round 1 lane 5": (9 + 1024 + 32 * 5,), "round 1 lane 52": (9 + 1024 + 32 * 20 + 4,),
          "two registers of one lane": (9 + 2048 + 32 * 7, 9 + 2048 + 32 * 7 + 1), "round 2": (9 + 2048 + 100,),
          "the partial last trip": (9 + 1024 * 10 + 500,), "tail": (11273 + 50,)}


@pytest.mark.parametrize("n_bins", (1, 7, 8, 9, 16))
def test_bin_edges_at_every_place(ctx, oracle, n_bins):
    """One k-mer W at a place; query 0 is W with n_bins - 1 bases changed (the window is counted, in the last bin), query 1 is W with n_bins
    changed (the window is counted nowhere).  6 / 7 / 8 probe the edge between the two tiers of eight bins, 15 / 16 the upper limit, 0 / 1 a
    histogram of one bin.  "two registers": the windows j and j + 1 of a run of k + 1 equal bases."""
    assert kw.scan_rounds(N_EDGE, 9) == 11
    rng = np.random.default_rng(40 + n_bins)
    k = K_EDGE
    base = rng.integers(0, 4, size=N_EDGE)
    for name, at in PLACES.items():
        codes = base.copy()
        if len(at) == 2:
            w = np.zeros(k, dtype=np.int64)
            codes[at[0] - 1], codes[at[0] + k + 1] = 1, 1
            codes[at[0]:at[0] + k + 1] = 0
        else:
            w = rng.integers(0, 4, size=k)
            codes[at[0]:at[0] + k] = w
        queries = np.array([ho.word(ho.substituted(rng, w, n_bins - 1)), ho.word(ho.substituted(rng, w, n_bins))], dtype=np.uint64)
        s = ho.ascii_of(rng, codes)
        d0, d1 = oracle.kmer_hdist_scan(s, k, int(queries[0])), oracle.kmer_hdist_scan(s, k, int(queries[1]))
        assert all(d0[p] == n_bins - 1 and d1[p] == n_bins for p in at), name
        want = np.stack([ho.truncated(d0, n_bins), ho.truncated(d1, n_bins)])
        assert want[0, n_bins - 1] >= len(at)
        a, p = _both(ctx, s, k, queries, n_bins, 7, 1)
        assert np.array_equal(a, want) and np.array_equal(p, want), (name, a, p, want)


def test_distance_k_has_a_bin_or_none(ctx, oracle):
    """d = k, the largest distance there is: a window that differs from the query in every base, counted with n_bins = k + 1 and not with n_bins = k"""
    rng = np.random.default_rng(12)
    k, n = 12, 6000
    codes = rng.integers(0, 4, size=n)
    qc = rng.integers(0, 4, size=k)
    for p in (2, 1500, 5900):
        codes[p:p + k] = (qc + 1 + rng.integers(0, 3, size=k)) & 3
    queries = np.array([ho.word(qc)], dtype=np.uint64)
    s = ho.ascii_of(rng, codes)
    d = oracle.kmer_hdist_scan(s, k, int(queries[0]))
    assert (d == k).sum() >= 3
    for n_bins in (k + 1, k):
        want = ho.truncated(d, n_bins)[None, :]
        a, p = _both(ctx, s, k, queries, n_bins, 1, 0)
        assert np.array_equal(a, want) and np.array_equal(p, want), n_bins
    assert int(ho.truncated(d, k + 1).sum()) == n - k + 1


# ---- 3. saturation and the flush period ----------------------------------------------------------------------------------------------------
FLUSH_TRIPS = 3  # scan_hist_device.h: kHistPeriod


def test_fields_do_not_saturate_over_many_trips(ctx):
    """Closed-form expectations, no oracle.  On a poly-A reference the query A^k with j bases changed puts EVERY window into bin j: a lane adds 64
    windows per trip to one 8-bit field, which wraps at the fourth trip unless the wave flushes every three.  ACAC... splits the windows between the
    bins j (even windows) and k (odd ones).  The size: every wave of the bounded grid (one workgroup of twelve waves per CU, trips of four rounds)
    walks seven trips -- two flush periods and a partial one -- and half of them an eighth.  Q = 17: two query blocks; k = 7 with 8 bins runs the
    one-tier kernels, k = 15 with 16 bins the two-tier ones."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = kw.pass_rounds(kw.kernels()["multi"], cus)
    rounds = (2 * FLUSH_TRIPS + 1) * R + R // 2
    n = rounds * 1024 + 32 + 1000
    assert kw.scan_rounds(n, 0) == rounds
    nq = 17
    for ref in ("A", "AC"):
        if ref == "A":
            t = torch.full((n + 16,), ord("A"), dtype=torch.uint8, device="cuda:0")
            words = torch.zeros((n + 31) // 32 + 2, dtype=torch.int64, device="cuda:0")
        else:
            t = torch.tensor([ord("A"), ord("C")], dtype=torch.uint8, device="cuda:0").repeat((n + 16) // 2)
            words = torch.full(((n + 31) // 32 + 2,), 0x4444444444444444, dtype=torch.int64, device="cuda:0")
        for k, n_bins in ((7, 8), (15, 16)):
            nwin = n - k + 1
            changes = [q % (k + 1) for q in range(nq)]
            queries, want = [], np.zeros((nq, n_bins), dtype=np.uint64)
            for q, j in enumerate(changes):
                qc = np.array([(i % 2) if ref == "AC" else 0 for i in range(k)])
                qc[:j] = 2 + (q % 2)  # G or T: in neither reference
                queries.append(ho.word(qc))
                if ref == "A":
                    want[q, j] += nwin
                else:
                    want[q, j] += (nwin + 1) // 2  # the even windows read ACAC...
                    want[q, k] += nwin // 2        # the odd ones CACA...: every base differs
            dq = _dev_queries(np.array(queries, dtype=np.uint64))
            b1, h1 = _output(nq, n_bins)
            b2, h2 = _output(nq, n_bins)
            torch.cuda.synchronize()
            ctx.kmer_hdist_hist_async(t, n, k, dq, nq, n_bins, h1)
            ctx.kmer_hdist_hist_packed_async(words, words.numel(), n, k, dq, nq, n_bins, h2)
            a, p = _read(ctx, b1, nq, n_bins), _read(ctx, b2, nq, n_bins)
            assert np.array_equal(a, want), (ref, k, np.argwhere(a != want)[:4], a[a != want][:4], want[a != want][:4])
            assert np.array_equal(p, want), (ref, k, np.argwhere(p != want)[:4], p[p != want][:4], want[p != want][:4])
        del t, words


# ---- 4. the identities with count_multi and best, on the device -------------------------------------------------------------------------------
def test_identities_with_count_multi_and_best_on_the_device(ctx, oracle):
    import torch
    rng = np.random.default_rng(404)
    n, nq = 10**6 + 7, 40
    for k, n_bins in ((31, 16), (12, 13), (23, 8)):
        queries = _queries(rng, nq, k)
        s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins, copies=400))
        want = ho.hist(oracle, s, k, queries, n_bins)
        ho.assert_rich(want, k, n_bins)
        t, ptr = _ascii_dev(s, 7)
        dq = _dev_queries(queries)
        b, hp = _output(nq, n_bins)
        counts = torch.zeros((n_bins, nq), dtype=torch.int64, device="cuda:0")
        taus = [torch.full((nq,), tt, dtype=torch.int32, device="cuda:0") for tt in range(n_bins)]
        pos = torch.zeros(nq, dtype=torch.int64, device="cuda:0")
        dist = torch.zeros(nq, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.kmer_hdist_hist_async(ptr, n, k, dq, nq, n_bins, hp)
        for tt in range(n_bins):
            ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, taus[tt], nq, counts[tt])
        ctx.kmer_hdist_best_async(ptr, n, k, dq, nq, pos, dist)
        h = _read(ctx, b, nq, n_bins)
        cm = counts.cpu().numpy().view(np.uint64)
        assert np.array_equal(np.cumsum(h, axis=1).T, cm), k
        bd = dist.cpu().numpy()
        for q in range(nq):
            nz = np.flatnonzero(h[q])
            assert (nz.size and nz[0] == bd[q]) if bd[q] < n_bins else nz.size == 0, (k, q)
        if n_bins > k:
            assert (h.sum(axis=1) == n - k + 1).all()
        assert np.array_equal(h, want)


# ---- 5. no windows, limits and argument errors ---------------------------------------------------------------------------------------------
def test_no_windows_limits_and_argument_errors(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(3)
    k, n, nq, n_bins = 17, 5000, 40, 9
    queries = _queries(rng, nq, k)
    s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
    t, ptr = _ascii_dev(s, 0)
    w = _pack(s)
    tw, wptr = _words_dev(w, 0)
    dq = _dev_queries(queries)
    dp = _dev_patterns(np.stack([po.from_2bit(int(q), k) for q in queries]))
    forms = ((lambda nn, kk, qq, b, h: ctx.kmer_hdist_hist_async(ptr, nn, kk, dq, qq, b, h)),
             (lambda nn, kk, qq, b, h: ctx.kmer_hdist_hist_packed_async(wptr, w.size, nn, kk, dq, qq, b, h)),
             (lambda nn, kk, qq, b, h: ctx.kmer_pattern_hist_async(ptr, nn, kk, dp, qq, b, h)),
             (lambda nn, kk, qq, b, h: ctx.kmer_pattern_hist_packed_async(wptr, w.size, nn, kk, dp, qq, b, h)))
    for form in forms:
        for kk, nn in ((k, k - 1), (0, n), (5, 0)):  # no windows: zeros in [0, nq * n_bins), nothing beside them
            buf, hp = _output(nq, n_bins)
            torch.cuda.synchronize()
            form(nn, kk, nq, n_bins, hp)
            assert (_read(ctx, buf, nq, n_bins) == 0).all()
        buf, hp = _output(nq, n_bins)
        torch.cuda.synchronize()
        form(n, k, 0, n_bins, hp)  # no queries: nothing written
        ctx.sync()
        assert bool((buf == FILL).all())
        ctx.sync()
        assert bool((buf == FILL).all())
    from bitnuc_amd import _lib as L
    buf, hp = _output(nq, n_bins)
    torch.cuda.synchronize()
    for name, head, qq in (("bitnuc_kmer_hdist_hist_async", (ptr, n), dq), ("bitnuc_kmer_hdist_hist_packed_async", (wptr, w.size, n), dq),
                           ("bitnuc_kmer_pattern_hist_async", (ptr, n), dp), ("bitnuc_kmer_pattern_hist_packed_async", (wptr, w.size, n), dp)):
        # the checks in their order: k, (packed: the words,) n_bins, n_queries, the arrays -- each with everything after it wrong as well
        st, e = _raw(ctx, name, *head, 33, qq, 65537, 17, hp + 4)
        assert st == L.SEQUENCE_TOO_LONG and e.value == 33
        for nb in (0, 17):
            st, e = _raw(ctx, name, *head, k, qq, 65537, nb, hp + 4)
            assert st == L.UNSUPPORTED and e.value == nb
        st, e = _raw(ctx, name, *head, k, qq, 65537, n_bins, hp + 4)
        assert st == L.UNSUPPORTED and e.value == 65537
        for q_arg, h_arg in ((qq, hp + 4), (qq, None), (None, hp), (qq.data_ptr() + 2, hp)):
            st, e = _raw(ctx, name, *head, k, q_arg, nq, n_bins, h_arg)
            assert st == L.UNSUPPORTED and e.value == 0
        st, e = _raw(ctx, name, *((None,) + head[1:]), k, qq, nq, n_bins, hp)  # a NULL reference: the last check
        assert st == L.UNSUPPORTED and e.value == 0
        st, e = _raw(ctx, name, *((None,) + head[1:-1] + (k - 1,)), k, qq, nq, n_bins, hp)  # ... after the no-window case: zeros
        assert st == L.OK
        assert (_read(ctx, buf, nq, n_bins) == 0).all()
        buf.fill_(FILL)
        torch.cuda.synchronize()
    ctx.sync()
    assert bool((buf == FILL).all())  # nothing written on an error
    with pytest.raises(bn.NucleotideError) as ei:  # packed: too few words, before the bins
        ctx.kmer_hdist_hist_packed_async(wptr, w.size - 1, n, k, dq, nq, 17, hp)
    assert ei.value.kind == "InvalidLength"
    del ei
    with pytest.raises(bn.NucleotideError):  # packed words not 8-byte aligned: the last check
        ctx.kmer_hdist_hist_packed_async(wptr + 4, w.size - 1, n - 64, k, dq, nq, n_bins, hp)
    with pytest.raises(bn.NucleotideError):  # a NULL reference
        ctx.kmer_hdist_hist_async(0, n, k, dq, nq, n_bins, hp)
    ctx.sync()
    assert bool((buf == FILL).all())


def test_the_query_limit(ctx, oracle):
    """BITNUC_MAX_QUERIES queries in one call (4096 query blocks) at a tiny n, against the host form in slices (the oracle on the first of them)."""
    from bitnuc_amd import api
    rng = np.random.default_rng(65536)
    k, n, nq, n_bins = 12, 3000, 65536, 9
    queries = _queries(rng, nq, k)
    s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
    free = api.context_free()
    first = ho.hist(oracle, s, k, queries[:64], n_bins)
    ho.assert_rich(first, k, n_bins)
    assert np.array_equal(free.kmer_hdist_hist(s, k, queries[:64], n_bins), first)
    full = np.concatenate([free.kmer_hdist_hist(s, k, queries[i:i + 256], n_bins) for i in range(0, nq, 256)])
    a, p = _both(ctx, s, k, queries, n_bins, 1, 1)
    assert np.array_equal(a, full) and np.array_equal(p, full)


# ---- 6. invalid bytes ----------------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_reported_once_with_the_first_index(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(5)
    k, n, nq, n_bins = 17, 50_000, 40, 9  # three query blocks: one of them reports
    queries = _queries(rng, nq, k)
    s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
    want = ho.hist(oracle, s, k, queries, n_bins)
    ho.assert_rich(want, k, n_bins)
    dq = _dev_queries(queries)
    for bad_at, off in ((31_337, 0), (n - 3, 5), (2, 9)):  # a middle round, the tail, the head
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        buf, hp = _output(nq, n_bins)
        torch.cuda.synchronize()
        ctx.kmer_hdist_hist_async(ptr, n, k, dq, nq, n_bins, hp)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing left for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean and correct
        buf, hp = _output(nq, n_bins)
        torch.cuda.synchronize()
        ctx.kmer_hdist_hist_async(ptr2, n, k, dq, nq, n_bins, hp)
        assert np.array_equal(_read(ctx, buf, nq, n_bins), want)


# ---- 7. hipGraph ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reference_and_the_queries_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(77)
    n, k, nq, n_bins = 300_001, 31, 33, 16
    q1, q2 = _queries(rng, nq, k), _queries(rng, nq, k)
    s1, s2 = ho.ascii_of(rng, ho.planted(rng, n, k, q1, n_bins, copies=200)), ho.ascii_of(rng, ho.planted(rng, n, k, q2, n_bins, copies=200))
    want1, want2 = ho.hist(oracle, s1, k, q1, n_bins), ho.hist(oracle, s2, k, q2, n_bins)
    ho.assert_rich(want1, k, n_bins)
    ho.assert_rich(want2, k, n_bins)
    assert not np.array_equal(want1, want2)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = _pack(s1)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        big = _dev_queries(_queries(rng, 4000, k))
        b1, h1 = _output(nq, n_bins)
        b2, h2 = _output(nq, n_bins)
        b3, h3 = _output(4000, n_bins)
        c.kmer_hdist_hist_async(ptr, n, k, dq, nq, n_bins, h1)  # warm-up outside the capture: sizes the scratch
        c.kmer_hdist_hist_packed_async(wptr, w.size, n, k, dq, nq, n_bins, h2)
        assert np.array_equal(_read(c, b1, nq, n_bins), want1) and np.array_equal(_read(c, b2, nq, n_bins), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.kmer_hdist_hist_async(ptr, n, k, dq, nq, n_bins, h1)
                c.kmer_hdist_hist_packed_async(wptr, w.size, n, k, dq, nq, n_bins, h2)
                # more queries than the warm-up's: the scratch would have to grow, which a capture cannot do -- refused, the capture survives
                with pytest.raises(bn.NucleotideError) as ei:
                    c.kmer_hdist_hist_packed_async(wptr, w.size, n, k, big, 4000, n_bins, h3)
                assert ei.value.kind == "Unsupported"
                del ei
                st_, e_ = _raw(c, "bitnuc_kmer_hdist_hist_async", ptr, n, k, big, 4000, n_bins, h3)
                assert st_ == 6 and e_.value >= 4000 * 2560  # Unsupported, with the bytes needed
            t[7:7 + n] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(_pack(s2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2))
            for _ in range(2):
                b1.fill_(FILL)
                b2.fill_(FILL)
                g.replay()
                assert np.array_equal(_read(c, b1, nq, n_bins), want2) and np.array_equal(_read(c, b2, nq, n_bins), want2)
            assert bool((b3 == FILL).all())
        finally:
            g.reset()
            del g
            c.close()


# ---- 8. a queue of mixed asynchronous calls --------------------------------------------------------------------------------------------------
def test_mixed_queue_with_one_sync(ctx, oracle):
    """hist and hist_packed (both tiers, exact and pattern) with best, count_multi, hits and reads_hdist_best between them on one context -- they
    share the stream and the scratch of the tables --, different query counts between consecutive calls, one sync at the end, every result checked
    afterwards."""
    import torch
    import reads_best_oracle as rbo
    rng = np.random.default_rng(606)
    k, n = 21, 70_001
    dev = torch.device("cuda:0")
    jobs = []
    for i, (nq, n_bins) in enumerate(((5, 8), (33, 16), (1, 9), (17, 3), (40, 16), (16, 7), (2, 12))):  # inputs and outputs first: torch's stream writes them
        queries = _queries(rng, nq, k)
        s = ho.ascii_of(rng, ho.planted(rng, n + i, k, queries, n_bins))
        taus = (np.arange(nq) % 5).astype(np.uint32)
        j = dict(i=i, nq=nq, n_bins=n_bins, queries=queries, s=s, taus=taus, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), w=_pack(s), dq=_dev_queries(queries),
                 dp=_dev_patterns(np.stack([po.from_2bit(int(q), k) for q in queries])), out=_output(nq, n_bins),
                 dt=torch.from_numpy(taus.view(np.int32)).to(dev), counts=torch.zeros(nq, dtype=torch.int64, device=dev),
                 hp=torch.zeros(64, dtype=torch.int64, device=dev), nh=torch.zeros(1, dtype=torch.int64, device=dev),
                 bpos=torch.zeros(nq, dtype=torch.int64, device=dev), bdist=torch.zeros(nq, dtype=torch.uint8, device=dev))
        j["wdev"] = _words_dev(j["w"], i & 1)
        j["reads"] = (s.size // 100, torch.zeros(s.size // 100, dtype=torch.int32, device=dev), torch.zeros(s.size // 100, dtype=torch.int32, device=dev),
                      torch.zeros(s.size // 100, dtype=torch.uint8, device=dev))
        jobs.append(j)
    torch.cuda.synchronize()
    calls = 0
    for j in jobs:  # the queue: nothing waits between these calls
        i, nq, n_bins, s, ptr, dq = j["i"], j["nq"], j["n_bins"], j["s"], j["ascii"][1], j["dq"]
        hptr = j["out"][1]
        if i % 4 == 0:
            ctx.kmer_hdist_hist_async(ptr, s.size, k, dq, nq, n_bins, hptr)
        elif i % 4 == 1:
            ctx.kmer_hdist_hist_packed_async(j["wdev"][1], j["w"].size, s.size, k, dq, nq, n_bins, hptr)
        elif i % 4 == 2:
            ctx.kmer_pattern_hist_async(ptr, s.size, k, j["dp"], nq, n_bins, hptr)
        else:
            ctx.kmer_pattern_hist_packed_async(j["wdev"][1], j["w"].size, s.size, k, j["dp"], nq, n_bins, hptr)
        if i % 4 == 0:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, j["bpos"], j["bdist"])
        elif i % 4 == 1:
            ctx.kmer_hdist_count_multi_dev(ptr, s.size, k, dq, j["dt"], nq, j["counts"])
        elif i % 4 == 2:
            ctx.kmer_hdist_hits_dev(ptr, s.size, k, int(j["queries"][0]), 3, j["hp"], None, 64, j["nh"])
        else:
            cnt, rq, rp, rd = j["reads"]
            ctx.reads_hdist_best_async(ptr, 100, cnt, k, dq, nq, rq, rp, rd)
        calls += 2
    assert calls >= 12
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, nq, n_bins, s, queries = j["i"], j["nq"], j["n_bins"], j["s"], j["queries"]
        want = ho.hist(oracle, s, k, queries, n_bins)
        ho.assert_rich(want, k, n_bins)
        assert np.array_equal(_read(ctx, j["out"][0], nq, n_bins), want), i
        d0 = oracle.kmer_hdist_scan(s, k, int(queries[0]))
        if i % 4 == 0:
            scans = [oracle.kmer_hdist_scan(s, k, int(q)) for q in queries]
            assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i
        elif i % 4 == 1:
            assert j["counts"].cpu().tolist() == [int(np.count_nonzero(oracle.kmer_hdist_scan(s, k, int(q)) <= int(t))) for q, t in zip(queries, j["taus"])], i
        elif i % 4 == 2:
            wh = np.nonzero(d0 <= 3)[0]
            assert int(j["nh"][0]) == wh.size and j["hp"].cpu().tolist()[:min(64, wh.size)] == list(wh[:64]), i
        else:
            cnt, rq, rp, rd = j["reads"]
            wq, wp, wd = rbo.reads_best(s[:cnt * 100], 100, cnt, k, queries)
            assert np.array_equal(rq.cpu().numpy().view(np.uint32), wq) and np.array_equal(rp.cpu().numpy().view(np.uint32), wp) and \
                np.array_equal(rd.cpu().numpy(), wd), i


# ---- 9. patterns ---------------------------------------------------------------------------------------------------------------------------
def test_pattern_singletons_equal_the_exact_forms_bit_for_bit(ctx, oracle):
    rng = np.random.default_rng(90)
    for k, n_bins, nq, n in ((31, 16, 17, 50_001), (8, 8, 5, 4129), (20, 9, 33, 10**5 + 3)):
        queries = _queries(rng, nq, k)
        s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins))
        want = ho.hist(oracle, s, k, queries, n_bins)
        ho.assert_rich(want, k, n_bins)
        singles = np.stack([po.from_2bit(int(q), k) for q in queries])
        ea, ep = _both(ctx, s, k, queries, n_bins, 1, 1)
        pa, pp = _both(ctx, s, k, singles, n_bins, 15, 0, patterns=True)
        assert np.array_equal(pa, ea) and np.array_equal(pp, ep) and np.array_equal(ea, want) and np.array_equal(ep, want)


def test_guides_with_ngg_against_the_pattern_oracle(ctx):
    """k = 23: twenty bases whose mismatches are counted, one N that never counts, GG that must match (a window without GG is two further away)"""
    rng = np.random.default_rng(23)
    k, n, nq = 23, 200_003, 18
    for n_bins in (4, 8, 16):
        guides = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=20)) + "NGG" for _ in range(nq)]
        pats = np.stack([po.from_iupac(g) for g in guides])
        qs = np.array([ho.word([po.CODE.get(ch, 2) for ch in g]) for g in guides], dtype=np.uint64)  # N -> G: some base
        codes = ho.planted(rng, n, k, qs, n_bins, copies=300)
        want = ho.pattern_hist(codes, pats, k, n_bins)
        ho.assert_rich(want, k, n_bins)
        a, p = _both(ctx, ho.ascii_of(rng, codes), k, pats, n_bins, 7, 1, patterns=True)
        assert np.array_equal(a, want) and np.array_equal(p, want), n_bins
    sets = [po.random_sets(rng, k) for _ in range(5)]  # empty sets and N among them
    pats = np.stack([po.from_sets(x) for x in sets])
    want = ho.pattern_hist(codes, pats, k, 16)
    a, p = _both(ctx, ho.ascii_of(rng, codes), k, pats, 16, 0, 0, patterns=True)
    assert np.array_equal(a, want) and np.array_equal(p, want)


# ---- 10. the host-pointer forms above the host cutoff ------------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context(oracle):
    """2 * 10^6 bases and three queries (6 * 10^6 window-query pairs, above the default cutoff of 2^20) on a context with the default dispatch: the
    four host forms and the PackedSequence methods run through the device in one chunk; the same call below the cutoff gives the oracle's answer too."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(808)
    n, k, n_bins = 2 * 10**6, 23, 10
    queries = _queries(rng, 3, k)
    s = ho.ascii_of(rng, ho.planted(rng, n, k, queries, n_bins, copies=500))
    want = ho.hist(oracle, s, k, queries, n_bins)
    ho.assert_rich(want, k, n_bins)
    singles = np.stack([po.from_2bit(int(q), k) for q in queries])
    c = bn.Context(0)
    try:
        assert (n - k + 1) * 3 >= 1 << 20
        assert np.array_equal(c.kmer_hdist_hist(s, k, queries, n_bins), want)
        assert np.array_equal(c.kmer_hdist_hist_packed(_pack(s), n, k, queries, n_bins), want)
        assert np.array_equal(c.kmer_pattern_hist(s, k, singles, n_bins), want)
        assert np.array_equal(c.kmer_pattern_hist_packed(_pack(s), n, k, singles, n_bins), want)
        seq = bn.PackedSequence(s, c)
        assert np.array_equal(seq.kmer_hdist_hist(k, queries, n_bins), want)
        assert np.array_equal(seq.kmer_pattern_hist(k, singles, n_bins), want)
        m = 100_000  # 3 * 10^5 pairs: the same call stays on the host
        assert np.array_equal(c.kmer_hdist_hist(s[:m], k, queries, n_bins), ho.hist(oracle, s[:m], k, queries, n_bins))
        b = s.copy()
        b[n - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.kmer_hdist_hist(b, k, queries, n_bins)
        assert (ei.value.byte, ei.value.index) == (ord("N"), n - 5)
        del ei
        assert np.array_equal(c.kmer_hdist_hist(s, k, queries, n_bins), want)  # the next call is clean
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff run in chunks of 128 Mi windows overlapping by k - 1 bases, summed per bin.  One query on 128 Mi + 3 M random
    bases with copies (d substitutions each) on both sides of the boundary and a run of A across it, whose windows -- the last of chunk 0, the first
    of chunk 1 and their neighbours -- fill the bins 0, 1, 2, ...: a window counted twice or not at all changes a bin by one.  Then an N past the boundary reports its
    absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1281)
    chunk = 128 << 20
    n, k, n_bins = chunk + 3_000_000, 25, 8
    codes = rng.integers(0, 4, size=n).astype(np.uint8)
    qc = np.zeros(k, dtype=np.int64)  # A^k: windows that overlap a run of A are all close to it
    for p, d in ((12_345, 0), (777, 7), (900, 8), (chunk - 5000, 1), (chunk + 200_000, 6), (n - k, 7)):
        codes[p:p + k] = ho.substituted(rng, qc, d)
    codes[chunk - 1:chunk + k] = 0  # k + 1 A between two C: the last window of chunk 0 (it reaches k - 1 bases into the halo) and the first of chunk 1
    codes[chunk - 2], codes[chunk + k] = 1, 1  # at distance 0, their neighbours on both sides at 1, 2, ... as the run leaves them
    s = LUT[codes]
    del codes
    queries = np.array([ho.word(qc) | (0xABC << (2 * k))], dtype=np.uint64)  # junk above 2k
    d = oracle.kmer_hdist_scan(s, k, int(queries[0]))
    want = ho.truncated(d, n_bins)[None, :]
    assert d[chunk - 1] == 0 and d[chunk] == 0 and d[chunk - 2] == 1 and d[chunk + 1] == 1 and d[n - k] == 7 and d[900] == 8
    del d
    ho.assert_rich(want, k, n_bins)
    assert np.array_equal(ctx.kmer_hdist_hist(s, k, queries, n_bins), want)
    assert np.array_equal(ctx.kmer_hdist_hist_packed(oracle.encode(s), n, k, queries, n_bins), want)
    s[chunk + 99] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_hist(s, k, queries, n_bins)
    assert (ei.value.byte, ei.value.index) == (ord("N"), chunk + 99)
    del ei


# ---- 11. beyond 2^32 -------------------------------------------------------------------------------------------------------------------------
def test_more_than_2_to_32_windows_in_one_bin(ctx):
    """poly-A, n = 2^32 + 2^20 + 37, the query A^k: hist[0] = n - k + 1 > 2^32 (closed form), packed and ASCII; with one base changed it moves to bin 1"""
    import torch
    dev = torch.device("cuda:0")
    n, k, n_bins = (1 << 32) + (1 << 20) + 37, 31, 3
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert free >= 6 << 30, f"needs 6 GiB of device memory: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB"
    nw = (n + 31) // 32
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    t = torch.full((n + 16,), ord("A"), dtype=torch.uint8, device=dev)
    for query, bin_ in ((0, 0), (3 << 10, 1)):
        dq = _dev_queries(np.array([query], dtype=np.uint64))
        b1, h1 = _output(1, n_bins)
        b2, h2 = _output(1, n_bins)
        torch.cuda.synchronize()
        ctx.kmer_hdist_hist_packed_async(words, nw, n, k, dq, 1, n_bins, h1)
        ctx.kmer_hdist_hist_async(t.data_ptr() + 1, n, k, dq, 1, n_bins, h2)
        want = [0] * n_bins
        want[bin_] = n - k + 1
        assert want[bin_] > 1 << 32
        assert _read(ctx, b1, 1, n_bins)[0].tolist() == want and _read(ctx, b2, 1, n_bins)[0].tolist() == want
    del t, words


# ---- 12. a seeded fuzz ---------------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(0xF0221)
    bad_cases = 0
    for case in range(200):
        k = int(rng.integers(1, 33))
        n = int(rng.choice((int(rng.integers(0, 200)), int(rng.integers(200, 5000)), int(rng.integers(5000, 70_001)))))
        nq = int(rng.choice((1, int(rng.integers(1, 18)), int(rng.integers(18, 41)))))
        n_bins = int(rng.integers(1, 17))
        packed, pattern = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        bad = case % 10 == 3  # a tenth of the cases: a planted invalid byte (and a later one), which only ASCII input with a window can hold
        if bad:
            packed, n = False, max(n, k)
        off = int(rng.integers(0, 16)) if not packed else int(rng.integers(0, 2))
        queries = _queries(rng, nq, k)
        codes = ho.planted(rng, n, k, queries, n_bins)
        s = ho.ascii_of(rng, codes)
        if pattern:
            q = np.stack([po.from_sets(po.random_sets(rng, k)) if i % 3 == 2 else po.from_2bit(int(x), k) for i, x in enumerate(queries)])
            want = ho.pattern_hist(codes, q, k, n_bins)
            dq = _dev_patterns(q)
        else:
            want = ho.hist(oracle, s, k, queries, n_bins)
            dq = _dev_queries(queries)
        bad_at = None
        if bad:
            bad_at = int(rng.integers(0, n))
            s = s.copy()
            s[bad_at] = rng.choice(np.frombuffer(b"N-x\x00\xff", dtype=np.uint8))
            s[n - 1] = ord("?") if bad_at < n - 1 else s[n - 1]
            bad_cases += 1
        buf, hp = _output(nq, n_bins)
        if packed:
            w = _pack(s)
            tw, wptr = _words_dev(w, off)
            fn = ctx.kmer_pattern_hist_packed_async if pattern else ctx.kmer_hdist_hist_packed_async
            torch.cuda.synchronize()
            fn(wptr, w.size, n, k, dq, nq, n_bins, hp)
        else:
            t, ptr = _ascii_dev(s, off)
            fn = ctx.kmer_pattern_hist_async if pattern else ctx.kmer_hdist_hist_async
            torch.cuda.synchronize()
            fn(ptr, n, k, dq, nq, n_bins, hp)
        if bad_at is None:
            got = _read(ctx, buf, nq, n_bins)
            assert np.array_equal(got, want), (case, k, n, nq, n_bins, packed, pattern, off)
        else:
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (int(s[bad_at]), bad_at), (case, k, n, off)
            del ei
    assert bad_cases == 20
