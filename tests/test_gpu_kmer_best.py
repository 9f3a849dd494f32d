"""GPU tests of the best match per query (bitnuc_kmer_hdist_best[_packed]_async, scan_best_device.h): dist[q] = the smallest distance of a window to
queries[q], pos[q] = the leftmost window that attains it, against the oracle's scan + np.argmin / np.min per query -- every k, sizes around the round /
trip / halo / tail boundaries, query counts around the query block of 16, ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed
words at 16-byte and 8-mod-16 offsets (rotating with k, so that every size meets every offset); ties between every pair of places a window can be computed at (head, lanes, registers, rounds, trips of one
wave and of several, workgroups, tail); guard bytes and words; the no-window fill; invalid bytes; a hipGraph replay after the reference and the
queries changed; a queue of mixed asynchronous calls with one sync; positions past 2^32; and the host-pointer forms above the host cutoff on a live
context, in one chunk and across the boundary of two."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1055, 1056, 1057, 4095, 4127, 4128, 4129, 10**6 + 7)
QS = (1, 2, 15, 16, 17, 33, 257)
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A
NO_POS = np.uint64(2**64 - 1)
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _seq(rng, n, k, queries):
    """n ASCII bases, about 30 % lowercase: copies of the queries with a few mutations, then random bases"""
    codes = rng.integers(0, 4, size=n)
    for i, q in enumerate(queries[:8]):
        p = int(rng.integers(0, max(n - k, 0) + 1)) if n >= k else 0
        qc = np.array([(int(q) >> (2 * b)) & 3 for b in range(k)])
        m = min(k, n - p)
        codes[p:p + m] = qc[:m]
        if i % 2 and m:
            codes[p + int(rng.integers(0, m))] = int(rng.integers(0, 4))
    s = LUT[codes]
    s[rng.random(n) < 0.3] |= 0x20
    return s.astype(np.uint8)


def _queries(rng, nq, k):
    """random queries with junk above 2k"""
    return rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=nq, dtype=np.uint64)


def _word(codes):
    return sum(int(c) << (2 * b) for b, c in enumerate(codes))


def _want(oracle, s, k, queries):
    """(pos, dist) by the oracle's scan and numpy's argmin / min (argmin returns the first minimum)"""
    nq = len(queries)
    if s.size < k or k == 0:
        return np.full(nq, NO_POS, dtype=np.uint64), np.full(nq, 0xFF, dtype=np.uint8)
    pos, dist = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint8)
    for i, q in enumerate(queries):
        d = oracle.kmer_hdist_scan(s, k, int(q))
        pos[i], dist[i] = np.argmin(d), np.min(d)
    return pos, dist


def _pack(s):
    """the packed words of an ASCII sequence (junk above 2n in the last word)"""
    n = s.size
    codes = (((s >> 1) ^ (s >> 2)) & 3).astype(np.uint64)
    nw = (n + 31) // 32
    pad = np.zeros(nw * 32, dtype=np.uint64)
    pad[:n] = codes
    w = np.bitwise_or.reduce(pad.reshape(nw, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1) if nw else np.zeros(0, dtype=np.uint64)
    if n % 32:
        w[-1] |= np.uint64(0xDEADBEEFCAFEF00D) & ~np.uint64((1 << (2 * (n % 32))) - 1)
    return w.astype(np.uint64)


def _dev_queries(queries):
    import torch
    return torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _outputs(nq, dist_off=1):
    """pos with guard words after pos[nq]; dist inside a guarded buffer, starting at byte dist_off of it"""
    import torch
    pos = torch.full((nq + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    dbuf = torch.full((dist_off + nq + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    return pos, dbuf, dbuf.data_ptr() + dist_off


def _read(ctx, pos, dbuf, nq, dist_off=1):
    ctx.sync()
    p = pos.cpu().numpy().view(np.uint64)
    d = dbuf.cpu().numpy()
    assert (p[nq:] == np.uint64(FILL)).all(), "pos written after n_queries"
    assert (d[:dist_off] == 0x5A).all() and (d[dist_off + nq:] == 0x5A).all(), "dist written outside [0, n_queries)"
    return p[:nq].copy(), d[dist_off:dist_off + nq].copy()


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


def _both(ctx, s, k, queries, off, woff):
    """((pos, dist) of the ASCII form, (pos, dist) of the packed form); dist at an odd byte offset, guards checked"""
    import torch
    n, nq = s.size, len(queries)
    t, ptr = _ascii_dev(s, off)
    w = _pack(s)
    tw, wptr = _words_dev(w, woff)
    assert wptr % 16 == 8 * woff
    dq = _dev_queries(queries)
    p1, b1, d1 = _outputs(nq)
    p2, b2, d2 = _outputs(nq)
    torch.cuda.synchronize()
    ctx.kmer_hdist_best_async(ptr, n, k, dq, nq, p1, d1)
    ctx.kmer_hdist_best_packed_async(wptr, w.size, n, k, dq, nq, p2, d2)
    got = _read(ctx, p1, b1, nq), _read(ctx, p2, b2, nq)
    del t, tw
    return got


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. every k, size, query count and offset -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_size_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(7100 + k)
    for si, n in enumerate(SIZES):
        nq = QS[(si + k) % len(QS)] if n < 10**6 else (33 if k % 2 else 17)
        queries = _queries(rng, nq, k)
        s = _seq(rng, n, k, queries)
        want = _want(oracle, s, k, queries)
        a, p = _both(ctx, s, k, queries, (0, 1, 7, 15)[(si + k) % 4], (si + k // 4) % 2)  # every (size, offset, parity) over the 32 k
        assert _same(a, want), (n, nq, np.nonzero((a[0] != want[0]) | (a[1] != want[1]))[0][:5])
        assert _same(p, want), (n, nq, np.nonzero((p[0] != want[0]) | (p[1] != want[1]))[0][:5])


@pytest.mark.parametrize("nq", QS)
def test_query_counts_at_one_size(ctx, oracle, nq):
    rng = np.random.default_rng(300 + nq)
    k, n = 20, 3 * 4096 + 1056 + 77
    queries = _queries(rng, nq, k)
    s = _seq(rng, n, k, queries)
    want = _want(oracle, s, k, queries)
    for off in (0, 1, 7, 15):
        a, p = _both(ctx, s, k, queries, off, off & 1)
        assert _same(a, want) and _same(p, want), off


# ---- 2. leftmost on ties -----------------------------------------------------------------------------------------------------------
K_TIE = 24
N_TIE = 3 * 4096 + 100
# ASCII at byte offset +7: the rounds start at window 9 (twelve rounds = three trips, one trip per wave), the tail at 9 + 12 * 1024 = 12297.
# A window's place in a round: 32 lane + 8 (register / 4) + 4 (lane / 32) + register % 4.
PLACES = {"head": 3, "round 0": 9 + 100, "round 1 lane 5": 9 + 1024 + 32 * 5, "round 1 lane 52": 9 + 1024 + 32 * 20 + 4, "round 2": 9 + 2048 + 100,
          "trip 1": 9 + 1024 * 5 + 333, "trip 2": 9 + 1024 * 9 + 77, "last round": 9 + 1024 * 11 + 1000 - K_TIE, "tail": 12330}


def _tie_case(ctx, oracle, base, k, p1, p2, off, woff):
    """copies of one k-mer at p1 < p2: the query itself (distance 0 twice) and the query with one base changed (distance 1 twice) must both report p1.
    The oracle says that no other window reaches those distances."""
    rng = np.random.default_rng(p1 * 31 + p2)
    qc = rng.integers(0, 4, size=k)
    near = qc.copy()
    near[k // 2] ^= 2
    codes = base.copy()
    codes[p1:p1 + k] = qc
    codes[p2:p2 + k] = qc
    s = LUT[codes].copy()
    s[rng.random(s.size) < 0.3] |= 0x20
    queries = np.array([_word(qc), _word(near)], dtype=np.uint64)
    for q, d0 in zip(queries, (0, 1)):
        d = oracle.kmer_hdist_scan(s, k, int(q))
        assert d.min() == d0 and list(np.nonzero(d <= 1)[0]) == [p1, p2], (p1, p2)
    a, p = _both(ctx, s, k, queries, off, woff)
    assert list(a[0]) == [p1, p1] and list(a[1]) == [0, 1], (p1, p2, a)
    assert list(p[0]) == [p1, p1] and list(p[1]) == [0, 1], (p1, p2, p)


def test_leftmost_wins_between_every_pair_of_places(ctx, oracle):
    base = np.random.default_rng(2024).integers(0, 4, size=N_TIE)
    places = sorted(PLACES.values())
    assert places[-1] + K_TIE <= N_TIE
    for i, p1 in enumerate(places):
        for p2 in places[i + 1:]:
            _tie_case(ctx, oracle, base, K_TIE, p1, p2, 7, 1)


def test_leftmost_wins_between_two_registers_of_one_lane(ctx, oracle):
    """Windows j and j + 1 (registers r and r + 1 of one lane): a run of k + 1 equal bases holds the query AAA...A twice at distance 0 and the query
    with one C twice at distance 1; the bases beside the run are C, so the windows beside the two are further away."""
    k = K_TIE
    codes = np.random.default_rng(77).integers(0, 4, size=N_TIE)
    for j in (9 + 2048 + 32 * 7, 9 + 1024 * 6 + 32 * 40 + 8 * 2 + 4 + 2, 4, 12340):  # registers 0 / 1, 10 / 11 of a lane; the head; the tail
        c = codes.copy()
        c[j - 1], c[j + k + 1] = 1, 1
        c[j:j + k + 1] = 0
        s = LUT[c].copy()
        near = np.zeros(k, dtype=np.int64)
        near[5] = 1
        queries = np.array([0, _word(near)], dtype=np.uint64)
        want = _want(oracle, s, k, queries)
        assert list(want[0]) == [j, j] and list(want[1]) == [0, 1]
        for q in queries:
            d = oracle.kmer_hdist_scan(s, k, int(q))
            assert list(np.nonzero(d == d.min())[0]) == [j, j + 1]
        a, p = _both(ctx, s, k, queries, 7, 1)
        assert _same(a, want) and _same(p, want), j


def test_leftmost_wins_between_workgroups(ctx, oracle):
    base = np.random.default_rng(99).integers(0, 4, size=10**6 + 7)
    _tie_case(ctx, oracle, base, K_TIE, 5000, 900_000, 0, 0)
    _tie_case(ctx, oracle, base, K_TIE, 123_456, 123_456 + 48 * 1024, 15, 1)  # the same wave and lane of the next workgroup


def test_leftmost_wins_between_the_trips_one_wave_walks(ctx, oracle):
    """A reference long enough for the bounded grid's waves to walk several trips (one workgroup per CU, twelve waves of four rounds each).  Three
    k-mers, each with the k-mer itself and the k-mer with one base changed as queries: copies at the same lane and register of one wave's first and
    second trip; of its second and third trip; and a copy with two changes in the first trip with the exact one in the third (the later, closer
    one wins)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride = cus * 12 * 4 * 1024  # windows between two trips of one wave
    n = 2 * stride + 3 * 10**6 + 11
    k = K_TIE
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 4, size=n)
    queries, want_pos, want_dist = [], [], []
    for i, (t1, t2, changes) in enumerate(((0, 1, 0), (1, 2, 0), (0, 2, 2))):
        p = 4096 * (37 + 5 * i) + 1024 * i + 32 * (9 + i) + 5
        qc = rng.integers(0, 4, size=k)
        first = qc.copy()
        first[[3, 17][:changes]] ^= 1
        near = qc.copy()
        near[9] ^= 3
        codes[p + t1 * stride:p + t1 * stride + k] = first
        codes[p + t2 * stride:p + t2 * stride + k] = qc
        queries += [_word(qc), _word(near)]
        want_pos += [p + (t2 if changes else t1) * stride] * 2
        want_dist += [0, 1]
    s = LUT[codes].copy()
    queries = np.array(queries, dtype=np.uint64)
    want = _want(oracle, s, k, queries)
    assert list(want[0]) == want_pos and list(want[1]) == want_dist
    a, pk = _both(ctx, s, k, queries, 0, 0)
    assert _same(a, want) and _same(pk, want)


# ---- 3. guards, fills and limits ---------------------------------------------------------------------------------------------------
def test_no_windows_fill_and_query_limits(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(3)
    k, n, nq = 17, 5000, 40
    queries = _queries(rng, nq, k)
    s = _seq(rng, n, k, queries)
    t, ptr = _ascii_dev(s, 0)
    w = _pack(s)
    tw, wptr = _words_dev(w, 0)
    dq = _dev_queries(queries)
    for dist_off in (1, 3, 8):
        for kk, nn in ((k, k - 1), (0, n), (5, 0)):  # no windows: the fill values, nothing beside them
            for packed in (False, True):
                pos, dbuf, dptr = _outputs(nq, dist_off)
                torch.cuda.synchronize()
                if packed:
                    ctx.kmer_hdist_best_packed_async(wptr, w.size, nn, kk, dq, nq, pos, dptr)
                else:
                    ctx.kmer_hdist_best_async(ptr, nn, kk, dq, nq, pos, dptr)
                p, d = _read(ctx, pos, dbuf, nq, dist_off)
                assert (p == NO_POS).all() and (d == 0xFF).all()
    pos, dbuf, dptr = _outputs(nq)
    torch.cuda.synchronize()
    ctx.kmer_hdist_best_async(ptr, n, k, dq, 0, pos, dptr)  # no queries: nothing written
    ctx.kmer_hdist_best_packed_async(wptr, w.size, n, k, dq, 0, pos, dptr)
    ctx.sync()
    assert bool((pos == FILL).all()) and bool((dbuf == 0x5A).all())
    for call in (lambda: ctx.kmer_hdist_best_async(ptr, n, k, dq, 65537, pos, dptr),
                 lambda: ctx.kmer_hdist_best_packed_async(wptr, w.size, n, k, dq, 65537, pos, dptr)):
        with pytest.raises(bn.NucleotideError) as ei:
            call()
        assert ei.value.kind == "Unsupported"
        del ei
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_best_async(ptr, n, 33, dq, nq, pos, dptr)
    assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
    del ei
    with pytest.raises(bn.NucleotideError):
        ctx.kmer_hdist_best_async(ptr, n, k, dq, nq, pos.data_ptr() + 4, dptr)
    with pytest.raises(bn.NucleotideError):
        ctx.kmer_hdist_best_packed_async(wptr + 4, w.size - 1, n - 64, k, dq, nq, pos, dptr)
    ctx.sync()
    assert bool((pos == FILL).all()) and bool((dbuf == 0x5A).all())


def test_the_query_limit(ctx, oracle):
    """BITNUC_MAX_QUERIES queries in one call (4096 query blocks) on a small reference, against the host form in slices."""
    from bitnuc_amd import api
    rng = np.random.default_rng(65536)
    k, n, nq = 12, 3000, 65536
    queries = _queries(rng, nq, k)
    s = _seq(rng, n, k, queries)
    free = api.context_free()
    assert _same(free.kmer_hdist_best(s, k, queries[:64]), _want(oracle, s, k, queries[:64]))
    parts = [free.kmer_hdist_best(s, k, queries[i:i + 256]) for i in range(0, nq, 256)]
    full = np.concatenate([p for p, _ in parts]), np.concatenate([d for _, d in parts])
    a, p = _both(ctx, s, k, queries, 1, 1)
    assert _same(a, full) and _same(p, full)


# ---- 4. invalid bytes --------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_reported_once_with_the_first_index(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(5)
    k, n, nq = 17, 50_000, 33
    queries = _queries(rng, nq, k)
    s = _seq(rng, n, k, queries)
    dq = _dev_queries(queries)
    for bad_at, off in ((31_337, 0), (n - 3, 5), (2, 9)):  # a middle round, the tail, the head
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        pos, dbuf, dptr = _outputs(nq)
        torch.cuda.synchronize()
        ctx.kmer_hdist_best_async(ptr, n, k, dq, nq, pos, dptr)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing left for the next sync
        t2, ptr2 = _ascii_dev(s, off)  # the next call on the same context is clean
        pos, dbuf, dptr = _outputs(nq)
        torch.cuda.synchronize()
        ctx.kmer_hdist_best_async(ptr2, n, k, dq, nq, pos, dptr)
        assert _same(_read(ctx, pos, dbuf, nq), _want(oracle, s, k, queries))


# ---- 5. hipGraph -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_reference_and_the_queries_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(77)
    n, k, nq = 300_001, 31, 33
    q1, q2 = _queries(rng, nq, k), _queries(rng, nq, k)
    s1, s2 = _seq(rng, n, k, q1), _seq(rng, n, k, q2)
    want1, want2 = _want(oracle, s1, k, q1), _want(oracle, s2, k, q2)
    assert not np.array_equal(want1[0], want2[0])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = _pack(s1)
        tw, wptr = _words_dev(w, 1)
        dq = _dev_queries(q1)
        p1, b1, d1 = _outputs(nq)
        p2, b2, d2 = _outputs(nq)
        c.kmer_hdist_best_async(ptr, n, k, dq, nq, p1, d1)  # warm-up outside the capture: sizes the scratch
        c.kmer_hdist_best_packed_async(wptr, w.size, n, k, dq, nq, p2, d2)
        assert _same(_read(c, p1, b1, nq), want1) and _same(_read(c, p2, b2, nq), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.kmer_hdist_best_async(ptr, n, k, dq, nq, p1, d1)
                c.kmer_hdist_best_packed_async(wptr, w.size, n, k, dq, nq, p2, d2)
            t[7:7 + n] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(_pack(s2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2))
            for _ in range(2):
                p1.fill_(FILL)
                p2.fill_(FILL)
                b1.fill_(0x5A)
                b2.fill_(0x5A)
                g.replay()
                assert _same(_read(c, p1, b1, nq), want2) and _same(_read(c, p2, b2, nq), want2)
        finally:
            g.reset()
            del g
            c.close()


# ---- 6. a queue of mixed asynchronous calls ------------------------------------------------------------------------------------------
def test_mixed_queue_with_one_sync(ctx, oracle):
    """best, best_packed, count_multi, hits, scan and encode enqueued on one context, different query counts between consecutive best calls (the
    scratch slot's keys and tables are rewritten by each), one sync at the end, every result checked afterwards."""
    import torch
    rng = np.random.default_rng(606)
    k, n = 21, 70_001
    dev = torch.device("cuda:0")
    jobs = []
    for i, nq in enumerate((5, 33, 1, 17, 40, 16, 2)):  # inputs and outputs first: torch's stream writes them
        queries = _queries(rng, nq, k)
        s = _seq(rng, n + i, k, queries)
        taus = (np.arange(nq) % 5).astype(np.uint32)
        jobs.append(dict(i=i, nq=nq, queries=queries, s=s, taus=taus, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), w=_pack(s), dq=_dev_queries(queries),
                         out=_outputs(nq), dt=torch.from_numpy(taus.view(np.int32)).to(dev), counts=torch.zeros(nq, dtype=torch.int64, device=dev),
                         hp=torch.zeros(64, dtype=torch.int64, device=dev), nh=torch.zeros(1, dtype=torch.int64, device=dev),
                         dist=torch.zeros(s.size - k + 1, dtype=torch.uint8, device=dev), words=torch.zeros((s.size + 31) // 32, dtype=torch.int64, device=dev)))
        jobs[-1]["wdev"] = _words_dev(jobs[-1]["w"], i & 1)
    torch.cuda.synchronize()
    calls = 0
    for j in jobs:  # the queue: nothing waits between these calls
        i, nq, s, ptr, dq = j["i"], j["nq"], j["s"], j["ascii"][1], j["dq"]
        pos, _, dptr = j["out"]
        if i % 2 == 0:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, pos, dptr)
        else:
            ctx.kmer_hdist_best_packed_async(j["wdev"][1], j["w"].size, s.size, k, dq, nq, pos, dptr)
        if i % 4 == 0:
            ctx.kmer_hdist_count_multi_dev(ptr, s.size, k, dq, j["dt"], nq, j["counts"])
        elif i % 4 == 1:
            ctx.kmer_hdist_hits_dev(ptr, s.size, k, int(j["queries"][0]), 3, j["hp"], None, 64, j["nh"])
        elif i % 4 == 2:
            ctx.kmer_hdist_scan_dev(ptr, s.size, k, int(j["queries"][0]), j["dist"])
        else:
            ctx.encode_dev(ptr, s.size, j["words"])
        calls += 2
    assert calls >= 12
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, nq, s, queries = j["i"], j["nq"], j["s"], j["queries"]
        pos, dbuf, _ = j["out"]
        assert _same(_read(ctx, pos, dbuf, nq), _want(oracle, s, k, queries)), i
        d0 = oracle.kmer_hdist_scan(s, k, int(queries[0]))
        if i % 4 == 0:
            assert j["counts"].cpu().tolist() == [int(np.count_nonzero(oracle.kmer_hdist_scan(s, k, int(q)) <= int(t))) for q, t in zip(queries, j["taus"])], i
        elif i % 4 == 1:
            wh = np.nonzero(d0 <= 3)[0]
            assert int(j["nh"][0]) == wh.size and j["hp"].cpu().tolist()[:min(64, wh.size)] == list(wh[:64]), i
        elif i % 4 == 2:
            assert np.array_equal(j["dist"].cpu().numpy(), d0), i
        else:
            assert np.array_equal(j["words"].cpu().numpy().view(np.uint64), oracle.encode(s)), i


# ---- 7. beyond 2^32 ------------------------------------------------------------------------------------------------------------------
def test_positions_beyond_32_bits(ctx, oracle):
    """2^32 + 5000 nucgen bases encoded on the device chunk by chunk; two queries that are windows of the stream at 2^32 + 1234 and 77 (their words
    from the closed-form stream, and the same bases read back from the device); a third one base off the first."""
    import torch
    dev = torch.device("cuda:0")
    n, k, seed = (1 << 32) + 5000, 31, 0xB17C0DE
    chunk = 1 << 30
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert free >= 3 * chunk, f"needs 3 GiB of device memory: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB"
    nw = (n + 31) // 32
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    buf = torch.empty(chunk, dtype=torch.uint8, device=dev)
    places = ((1 << 32) + 1234, 77)
    on_device = {}
    torch.cuda.synchronize()
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        ctx.nucgen_dev(buf, m, seed, first=i0)
        ctx.encode_dev(buf, m, words[i0 // 32:])
        ctx.sync()
        for p in places:
            if i0 <= p and p + k <= i0 + m:
                on_device[p] = buf[p - i0:p - i0 + k].cpu().numpy()
    queries = []
    for p in places:
        h = oracle.nucgen(k, seed, first=p)
        assert np.array_equal(h, on_device[p])
        queries.append(_word(((h >> 1) ^ (h >> 2)) & 3))
    queries.append(queries[0] ^ (2 << 20))  # one base of the first changed
    dq = _dev_queries(np.array(queries, dtype=np.uint64))
    pos, dbuf, dptr = _outputs(3)
    torch.cuda.synchronize()
    ctx.kmer_hdist_best_packed_async(words, nw, n, k, dq, 3, pos, dptr)
    p, d = _read(ctx, pos, dbuf, 3)
    assert list(p) == [places[0], places[1], places[0]] and list(d) == [0, 0, 1]


# ---- 8. the host-pointer forms above the host cutoff -------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context(oracle):
    """2 * 10^6 bases and three queries (6 * 10^6 window-query pairs, above the default cutoff of 2^20) on a context with the default dispatch:
    Context.kmer_hdist_best, .kmer_hdist_best_packed and PackedSequence.kmer_hdist_best run through the device in one chunk; the same calls below the
    cutoff and one query passed as a number give the same answers."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(808)
    n, k = 2 * 10**6, 23
    queries = _queries(rng, 3, k)
    s = _seq(rng, n, k, queries)
    want = _want(oracle, s, k, queries)
    c = bn.Context(0)
    try:
        assert (n - k + 1) * 3 >= 1 << 20
        assert _same(c.kmer_hdist_best(s, k, queries), want)
        assert _same(c.kmer_hdist_best_packed(_pack(s), n, k, queries), want)
        seq = bn.PackedSequence(s, c)
        assert _same(seq.kmer_hdist_best(k, queries), want)
        one = c.kmer_hdist_best(s, k, int(queries[1]))  # a scalar query: Q = 1
        assert one[0].shape == (1,) and (one[0][0], one[1][0]) == (want[0][1], want[1][1])
        m = 100_000  # 3 * 10^5 pairs: the same call stays on the host
        assert _same(c.kmer_hdist_best(s[:m], k, queries), _want(oracle, s[:m], k, queries))
        b = s.copy()
        b[n - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.kmer_hdist_best(b, k, queries)
        assert (ei.value.byte, ei.value.index) == (ord("N"), n - 5)
        del ei
        assert _same(c.kmer_hdist_best(s, k, queries), want)  # the next call is clean
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff run in chunks of 128 Mi windows overlapping by k - 1 bases, merged by the smallest (dist, absolute position).
    Five queries on 128 Mi + 3 M random bases (whose windows stay further than 3 from the four planted k-mers: checked with the oracle's scans):
      0  exact copies just before the boundary and after it: the equal distance of chunk 1 must not displace chunk 0's position;
      1  a copy with two changes in chunk 0, the exact one in chunk 1: the strictly closer one wins, with its absolute position;
      2  copies with one change at window chunk - 10 (the last windows of chunk 0 reach into the halo) and in chunk 1: the first one;
      3  one change early, exact at the last window n - k;
      4  a random query with junk above 2k: whatever the oracle says.
    Then an N past the boundary reports its absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1281)
    chunk = 128 << 20
    n, k = chunk + 3_000_000, 25
    codes = rng.integers(0, 4, size=n).astype(np.uint8)
    kmers = [rng.integers(0, 4, size=k) for _ in range(4)]

    def changed(qc, at):
        c = qc.copy()
        c[list(at)] ^= 1
        return c

    plan = ((0, chunk - 5000, ()), (0, chunk + 7000, ()),
            (1, 12_345, (3, 17)), (1, chunk + 200_000, ()),
            (2, chunk - 10, (11,)), (2, chunk + 1_000_000, (4,)),
            (3, 777, (20,)), (3, n - k, ()))
    for qi, p, at in plan:
        codes[p:p + k] = changed(kmers[qi], at)
    s = LUT[codes]
    del codes
    queries = np.array([_word(q) for q in kmers] + [int(_queries(rng, 1, k)[0])], dtype=np.uint64)
    queries[:4] |= np.uint64(0xABC) << np.uint64(2 * k)  # junk above 2k
    want = np.empty(5, dtype=np.uint64), np.empty(5, dtype=np.uint8)
    for qi in range(5):  # one oracle scan per query
        d = oracle.kmer_hdist_scan(s, k, int(queries[qi]))
        want[0][qi], want[1][qi] = np.argmin(d), np.min(d)
        if qi < 4:  # nothing but the planted copies comes near: the answers below do not rest on chance
            assert sorted(np.nonzero(d <= 3)[0]) == sorted(p for q, p, _ in plan if q == qi), qi
        del d
    assert list(want[0][:4]) == [chunk - 5000, chunk + 200_000, chunk - 10, n - k] and list(want[1][:4]) == [0, 0, 1, 0]
    assert _same(ctx.kmer_hdist_best(s, k, queries), want)
    assert _same(ctx.kmer_hdist_best_packed(oracle.encode(s), n, k, queries), want)
    s[chunk + 99] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_best(s, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("N"), chunk + 99)
    del ei
