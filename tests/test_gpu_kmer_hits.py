"""GPU tests of the k-mer hit lists (bitnuc_kmer_hdist_hits*, scan_hits_device.h): the positions of the windows with distance <= tau, in
ascending order, and their distances, against np.flatnonzero over the oracle's scan -- every k, sizes around the round / trip / halo / tail
boundaries, the tau range, ASCII at byte offsets +0 / +1 / +7 / +15 and packed words at 16-byte and 8-mod-16 offsets; the cap contract with guard
bytes; *n_hits against the count; invalid bytes and argument errors as the count reports them; a hipGraph replay; the host forms across the host
chunk; and 10^9 bases at k = 31 against the library's dense scan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1055, 1056, 1057, 2079, 4095, 4096 + 31, 4096 + 32, 4096 + 33, 4 * 4096 + 1056 + 17, 10**5 + 7)
GUARD = 64
POS_FILL = 0x5A5A5A5A5A5A5A5A
DIST_FILL = 0xEE


def _taus(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 2**32 - 1})


def _ascii(rng, n, k, dense):
    """n ASCII bases (mixed case) and a query; dense: mostly copies of the query (most windows within a small distance)"""
    q = rng.integers(0, 4, size=k)
    query = int(sum(int(c) << (2 * i) for i, c in enumerate(q))) | (int(rng.integers(0, 2**32)) << 2 * k if k < 32 else 0)
    codes = np.resize(q, n) if dense else rng.integers(0, 4, size=n)
    if dense and n:
        flip = rng.random(n) < 0.05
        codes[flip] = rng.integers(0, 4, size=int(flip.sum()))
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = lut[codes]
    low = rng.random(n) < 0.3
    s[low] |= 0x20
    return s.astype(np.uint8), query & (2**64 - 1)


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


def _buffers(cap, with_dist):
    import torch
    pos = torch.full((cap + GUARD,), POS_FILL, dtype=torch.int64, device="cuda:0")
    dist = torch.full((cap + GUARD,), DIST_FILL, dtype=torch.uint8, device="cuda:0") if with_dist else None
    nh = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    return pos, dist, nh


def _read(ctx, pos, dist, nh, cap):
    ctx.sync()
    total = int(nh.cpu()[0])
    p = pos.cpu().numpy().view(np.uint64)
    assert (p[cap:] == np.uint64(POS_FILL)).all(), "positions written at or beyond cap"
    d = None
    if dist is not None:
        d = dist.cpu().numpy()
        assert (d[cap:] == DIST_FILL).all(), "distances written at or beyond cap"
    got = min(cap, total)
    return total, p[:got], (d[:got] if d is not None else None)


def _ascii_dev(ctx, s, off):
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


def _hits_ascii(ctx, ptr, n, k, query, tau, cap, with_dist=True):
    import torch
    pos, dist, nh = _buffers(cap, with_dist)
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_dev(ptr, n, k, query, tau, pos, dist, cap, nh)
    return _read(ctx, pos, dist, nh, cap)


def _hits_packed(ctx, wptr, nw, n, k, query, tau, cap, with_dist=True):
    import torch
    pos, dist, nh = _buffers(cap, with_dist)
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_packed_dev(wptr, nw, n, k, query, tau, pos, dist, cap, nh)
    return _read(ctx, pos, dist, nh, cap)


def _check(want_d, tau, total, p, d):
    want = np.flatnonzero(want_d <= tau)
    assert total == want.size
    assert np.array_equal(p, want.astype(np.uint64)), int(np.nonzero(p != want.astype(np.uint64))[0][0]) if p.size == want.size else (p.size, want.size)
    if d is not None:
        assert np.array_equal(d, want_d[want])


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_size_tau_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(7000 + k)
    for si, n in enumerate(SIZES):
        for dense in (False, True):
            s, query = _ascii(rng, n, k, dense)
            want_d = oracle.kmer_hdist_scan(s, k, query) if n >= k else np.zeros(0, dtype=np.uint8)
            nwin = want_d.size
            off = (0, 1, 7, 15)[(si + dense) % 4]
            t, ptr = _ascii_dev(ctx, s, off)
            w = _pack(s)
            woff = (si + dense) % 2
            tw, wptr = _words_dev(w, woff)
            assert wptr % 16 == 8 * woff
            for tau in _taus(k):
                cap = nwin + 5
                _check(want_d, tau, *_hits_ascii(ctx, ptr, n, k, query, tau, cap, with_dist=(tau & 1) == 0 or tau > 33))
                _check(want_d, tau, *_hits_packed(ctx, wptr, w.size, n, k, query, tau, cap, with_dist=(tau & 1) == 1 or tau > 33))
            del t, tw


def test_every_byte_offset_of_ascii_input(ctx, oracle):
    rng = np.random.default_rng(77)
    k, n = 21, 3 * 4096 + 1056 + 100
    s, query = _ascii(rng, n, k, True)
    want_d = oracle.kmer_hdist_scan(s, k, query)
    for off in range(16):
        t, ptr = _ascii_dev(ctx, s, off)
        _check(want_d, 4, *_hits_ascii(ctx, ptr, n, k, query, 4, want_d.size))


def test_cap_contract_and_count_agreement(ctx, oracle):
    import torch
    rng = np.random.default_rng(5)
    for k, n, dense, tau in ((31, 5 * 4096 + 777, True, 6), (12, 70_001, False, 3), (5, 3000, True, 1)):
        s, query = _ascii(rng, n, k, dense)
        want_d = oracle.kmer_hdist_scan(s, k, query)
        want = np.flatnonzero(want_d <= tau)
        total = want.size
        assert total > 2
        t, ptr = _ascii_dev(ctx, s, 3)
        w = _pack(s)
        tw, wptr = _words_dev(w, 1)
        cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.kmer_hdist_count_dev(ptr, n, k, query, tau, cnt.data_ptr())
        ctx.kmer_hdist_count_packed_dev(wptr, w.size, n, k, query, tau, cnt.data_ptr() + 8)
        ctx.sync()
        assert [int(x) for x in cnt.cpu()] == [total, total]
        for cap in (0, 1, total - 1, total, total + 5):
            for with_dist in (False, True):
                for got in (_hits_ascii(ctx, ptr, n, k, query, tau, cap, with_dist), _hits_packed(ctx, wptr, w.size, n, k, query, tau, cap, with_dist)):
                    tot, p, d = got
                    assert tot == total
                    m = min(cap, total)
                    assert np.array_equal(p, want[:m].astype(np.uint64))
                    if with_dist:
                        assert np.array_equal(d, want_d[want[:m]])
        # deterministic: the same call gives the same bytes
        a = _hits_ascii(ctx, ptr, n, k, query, tau, total)
        b = _hits_ascii(ctx, ptr, n, k, query, tau, total)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # cap 0 with NULL pointers
    s, query = _ascii(rng, 5000, 9, True)
    t, ptr = _ascii_dev(ctx, s, 0)
    nh = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_dev(ptr, s.size, 9, query, 2, None, None, 0, nh)
    ctx.sync()
    assert int(nh.cpu()[0]) == int((oracle.kmer_hdist_scan(s, 9, query) <= 2).sum())


def test_invalid_byte_reported_as_the_count_reports_it(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(9)
    k, n = 17, 6 * 4096 + 1056 + 300
    base, query = _ascii(rng, n, k, False)
    # a round boundary, a trip boundary, inside a trip's halo, the tail, the head before the aligned base, and two at once (the first wins)
    for plant in ((1024,), (4096,), (4096 + 5,), (4095,), (n - 3,), (2,), (3 * 4096 + 9, 8193)):
        s = base.copy()
        for p in plant:
            s[p] = ord("N")
        for off in (0, 5):
            t, ptr = _ascii_dev(ctx, s, off)
            pos, dist, nh = _buffers(n, True)
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.kmer_hdist_count_dev(ptr, n, k, query, 3, cnt)
            with pytest.raises(bn.NucleotideError) as e1:
                ctx.sync()
            want = (e1.value.byte, e1.value.index)
            del e1
            ctx.kmer_hdist_hits_dev(ptr, n, k, query, 3, pos, dist, n, nh)
            with pytest.raises(bn.NucleotideError) as e2:
                ctx.sync()
            assert (e2.value.byte, e2.value.index) == want == (ord("N"), min(plant)), (plant, off)
            del e2


def test_argument_errors_in_order(ctx):
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L
    ref = torch.full((4096,), ord("A"), dtype=torch.uint8, device="cuda:0")
    words = torch.zeros(130, dtype=torch.int64, device="cuda:0")
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    P, NH = buf.data_ptr(), buf.data_ptr() + 8 * 4000

    def kind(fn, *a):
        try:
            fn(*a)
        except bn.NucleotideError as e:
            return e.kind, dict(e.payload)
        return "ok", {}
    h, hp = ctx.kmer_hdist_hits_dev, ctx.kmer_hdist_hits_packed_dev
    assert kind(h, ref, 4096, 33, 0, 1, P, None, 10, NH) == ("SequenceTooLong", {"len": 33})
    assert kind(h, ref, 4096, 33, 0, 1, P + 1, None, 10, NH + 1)[0] == "SequenceTooLong"  # k first
    assert kind(h, ref, 4096, 31, 0, 1, P, None, 10, NH + 4)[0] == "Unsupported"
    assert kind(h, ref, 4096, 31, 0, 1, P, None, 10, None)[0] == "Unsupported"
    assert kind(h, ref, 4096, 31, 0, 1, P + 4, None, 10, NH)[0] == "Unsupported"
    assert kind(h, ref, 4096, 31, 0, 1, None, None, 10, NH)[0] == "Unsupported"
    assert kind(h, None, 4096, 31, 0, 1, P, None, 10, NH)[0] == "Unsupported"
    assert kind(h, None, 10, 31, 0, 1, P, None, 10, NH) == ("ok", {})  # no windows before the reference pointer
    assert kind(h, ref, 4096, 31, 0, 1, None, None, 0, NH) == ("ok", {})
    assert kind(hp, words, 130, 4096, 33, 0, 1, P, None, 10, NH) == ("SequenceTooLong", {"len": 33})
    assert kind(hp, words, 127, 4096, 31, 0, 1, P, None, 10, NH) == ("InvalidLength", {"len": 4096})
    assert kind(hp, words.data_ptr() + 4, 130, 4096, 31, 0, 1, P, None, 10, NH)[0] == "Unsupported"
    assert kind(hp, words, 130, 4096, 31, 0, 1, P, None, 10, NH + 4)[0] == "Unsupported"
    assert kind(hp, words, 130, 4096, 31, 0, 1, None, None, 10, NH)[0] == "Unsupported"
    assert kind(hp, words, 130, 4096, 31, 0, 1, P, None, 10, NH) == ("ok", {})
    ctx.sync()
    nh = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    h(ref, 20, 31, 0, 1, P, None, 10, nh)  # n < k: *n_hits = 0
    ctx.sync()
    assert int(nh.cpu()[0]) == 0
    assert L.UNSUPPORTED


def test_graph_replay_matches_the_direct_call(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(31)
    n, k, tau = 2_000_003, 31, 12
    s, query = _ascii(rng, n, k, True)
    want_d = oracle.kmer_hdist_scan(s, k, query)
    want = np.flatnonzero(want_d <= tau)
    w = _pack(s)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(c, s, 7)
        tw, wptr = _words_dev(w, 1)
        cap = want.size + 3
        pos = torch.zeros((2, cap), dtype=torch.int64, device="cuda:0")
        dist = torch.zeros((2, cap), dtype=torch.uint8, device="cuda:0")
        nh = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        c.kmer_hdist_hits_dev(ptr, n, k, query, tau, pos[0], dist[0], cap, nh)  # warm-up outside the capture: sizes the scratch
        c.kmer_hdist_hits_packed_dev(wptr, w.size, n, k, query, tau, pos[1], dist[1], cap, nh.data_ptr() + 8)
        c.sync()
        direct = (pos.cpu().numpy().copy(), dist.cpu().numpy().copy(), nh.cpu().numpy().copy())
        assert list(direct[2]) == [want.size, want.size]
        assert np.array_equal(direct[0][0, :want.size].astype(np.uint64), want) and np.array_equal(direct[0][1], direct[0][0])
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.kmer_hdist_hits_dev(ptr, n, k, query, tau, pos[0], dist[0], cap, nh)
                c.kmer_hdist_hits_packed_dev(wptr, w.size, n, k, query, tau, pos[1], dist[1], cap, nh.data_ptr() + 8)
            for _ in range(2):
                pos.fill_(-1)
                dist.fill_(0)
                nh.fill_(-1)
                g.replay()
                c.sync()
                m = want.size
                hp, hd = pos.cpu().numpy(), dist.cpu().numpy()
                assert np.array_equal(hp[:, :m], direct[0][:, :m]) and np.array_equal(hd[:, :m], direct[1][:, :m])
                assert (hp[:, m:] == -1).all() and (hd[:, m:] == 0).all()  # nothing past the hits
                assert np.array_equal(nh.cpu().numpy(), direct[2])
        finally:
            g.reset()
            del g
            c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff: chunks of 128 M windows overlapping by k - 1 bases; hits planted across the chunk boundary."""
    rng = np.random.default_rng(11)
    chunk = 128 << 20
    n, k = chunk + 5_000_000, 25
    s, query = _ascii(rng, n, k, False)
    qb = np.frombuffer(b"ACGT", dtype=np.uint8)[[(query >> (2 * i)) & 3 for i in range(k)]]
    # copies of the query that do not overlap: the last windows of the first chunk (the last one reads k - 1 bases of the second), the first ones
    # of the second
    for p in (12345, chunk - 2 * k - 5, chunk - k - 1, chunk - 1, chunk + k, chunk + 2 * k + 3, n - k):
        s[p:p + k] = qb
    want_d = oracle.kmer_hdist_scan(s, k, query)
    w = oracle.encode(s)
    for tau in (0, 3):
        want = np.flatnonzero(want_d <= tau)
        assert want.size >= 7 and chunk - 1 in set(want.tolist())
        p, d = ctx.kmer_hdist_hits(s, k, query, tau, with_dist=True)
        assert np.array_equal(p, want.astype(np.uint64)) and np.array_equal(d, want_d[want])
        p2 = ctx.kmer_hdist_hits_packed(w, n, k, query, tau)
        assert np.array_equal(p2, want.astype(np.uint64))
    # invalid byte in the second chunk, as the host count of positions reports it
    import bitnuc_amd as bn
    s[chunk + 99] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_hits(s, k, query, 3)
    assert (ei.value.byte, ei.value.index) == (ord("N"), chunk + 99)
    del ei


def test_full_size_against_the_dense_scan_and_the_count(ctx):
    """10^9 nucgen bases, k = 31, the query at base 777,777,777: the hit lists (ASCII and packed) at tau 3, 8, 20 against flatnonzero(dist <= tau)
    over the library's dense scan (oracle-checked at this size by test_gpu_packed_scan / test_gpu_fullsize) and against the count."""
    import torch
    dev = torch.device("cuda:0")
    n, k, qpos = 10**9, 31, 777_777_777
    nwin = n - k + 1
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, 0xB17C0DE)
    ctx.sync()
    h = ref[qpos:qpos + k].cpu().numpy()
    query = int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h)))
    nw = (n + 31) // 32
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    dist = torch.empty(nwin, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.encode_dev(ref, n, words)
    ctx.kmer_hdist_scan_dev(ref, n, k, query, dist)
    ctx.sync()
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    nh = torch.zeros(2, dtype=torch.int64, device=dev)
    for tau in (3, 8, 20):
        want = torch.nonzero(dist <= tau).flatten()
        total = want.numel()
        cap = total + 5
        pos = torch.full((2, cap + GUARD), -7, dtype=torch.int64, device=dev)
        hd = torch.full((2, cap + GUARD), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.kmer_hdist_count_dev(ref, n, k, query, tau, cnt)
        ctx.kmer_hdist_hits_dev(ref, n, k, query, tau, pos[0], hd[0], cap, nh)
        ctx.kmer_hdist_hits_packed_dev(words, nw, n, k, query, tau, pos[1], hd[1], cap, nh.data_ptr() + 8)
        ctx.sync()
        assert int(cnt[0]) == total and [int(x) for x in nh.cpu()] == [total, total], tau
        for f in range(2):
            assert torch.equal(pos[f, :total], want), (tau, f)
            assert torch.equal(hd[f, :total], dist[want]), (tau, f)
            assert bool((pos[f, total:] == -7).all()) and bool((hd[f, total:] == 0xEE).all())
        if tau == 3:
            assert qpos in set(want.cpu().tolist())
        del pos, hd, want
