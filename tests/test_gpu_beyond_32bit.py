"""GPU tests of the k-mer kernels at window indices, byte offsets, ranks and counts past 32 bits: the aligned and unaligned ASCII scans, the
fused counts, the hit lists (ASCII at +0 / +1 / +7, packed words at 16-byte and 8-mod-16 offsets) and the packed scan and count on 2^32 + 2^20 + 37
bases; the hit lists' scan of the per-trip counts over more than 2048 tiles (three chunks of hits_scan_top_kernel) on 2^35 + 2^26 + 19 packed
bases; the sliding window batches at strides 1, 2, 4, 16, 5 and 12; split_packed past base 2^32.

Full-length references are computed on the device (the library's aligned dense scan, itself checked against the oracle around 2^32, at the
tail and at every planted copy of the query) and compared in chunks of at most 2^30 elements; only small windows go to the CPU oracle.  Each
test checks the free device memory first and fails with the numbers if there is not enough (a skip would hide the point of the test)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P32 = 1 << 32
N_A = P32 + (1 << 20) + 37           # the ASCII sequence of sections A, B, D, E
N_C = (1 << 35) + (1 << 26) + 19     # the packed poly-A sequence of section C
K = 31
SEED = 0xB17C0DE
STEP = 1 << 30                       # elements per chunk of a comparison on the device (torch.nonzero / torch.equal temporaries)
GUARD = 64
POS_FILL = 0x5A5A5A5A5A5A5A5A
DIST_FILL = 0xEE
TAUS = (3, 12, 30, 31, 2**32 - 1)
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
MUT = (3, 14, 25)                    # the bases a near copy of the query changes (1, 2 or 3 of them)


def _dev():
    import torch
    return torch.device("cuda:0")


def _need(nbytes, what):
    import torch
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert free >= nbytes, f"{what} needs {nbytes / 2**30:.1f} GiB of device memory: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB"
    torch.cuda.reset_peak_memory_stats()


def _done(what):
    import torch
    print(f"{what}: peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB allocated")
    torch.cuda.empty_cache()


def _codes(b):
    """2-bit codes of ASCII bases (either case), numpy or torch"""
    return ((b >> 1) ^ (b >> 2)) & 3


def _copy_of(query, k, m):
    """the query's k bases as upper-case ASCII, with m of them changed (Hamming distance m)"""
    c = np.array([(query >> (2 * i)) & 3 for i in range(k)], dtype=np.uint8)
    for i in MUT[:m]:
        c[i] = (c[i] + 1) & 3
    return LUT[c]


def _chunks(total, step=STEP):
    for i in range(0, total, step):
        yield i, min(step, total - i)


def _equal(a, b):
    import torch
    assert a.numel() == b.numel()
    return all(torch.equal(a[i:i + m], b[i:i + m]) for i, m in _chunks(a.numel()))


def _count_le(dist, tau):
    t = min(tau, 32)  # a distance is at most 32
    return sum(int((dist[i:i + m] <= t).sum()) for i, m in _chunks(dist.numel()))


def _nonzero_le(dist, tau):
    import torch
    t = min(tau, 32)
    return torch.cat([torch.nonzero(dist[i:i + m] <= t).flatten() + i for i, m in _chunks(dist.numel())])


def _ascii_reference(ctx, oracle):
    """N_A nucgen bases (lower-case mix) + 16 spare bytes, a query copied from past 2^32, exact and near copies of it planted across 2^32, on a trip
    boundary of the aligned rounds and of the +1 / +7 views' rounds (skip 15 / 9: 16 + 4096 t), across a round boundary, in the last round and
    in the tail; the library's aligned dense scan of it, checked against the oracle around 2^32, over the last 4000 windows and at every plant.
    -> seq, dist, query, planted window positions"""
    import torch
    n, k = N_A, K
    nwin = n - k + 1
    seq = torch.empty(n + 16, dtype=torch.uint8, device=_dev())
    ctx.nucgen_dev(seq, n, SEED, flags=2)
    ctx.sync()
    qpos = P32 + (1 << 19) + 123
    query = int(sum(int(c) << (2 * i) for i, c in enumerate(_codes(seq[qpos:qpos + k].cpu().numpy()))))
    plants = [(P32 - 13, 0), (P32 + 4096 * 40, 0), (P32 + 4096 * 50 + 1024 - 10, 2), (P32 + 16 + 4096 * 60 - 5, 1), (P32 + 4096 * 70 + 3, 3),
              (n - k - 100, 3), (n - k, 0)]
    assert n - k >= 1024 * ((n - 32) >> 10)  # the last window is a tail window of the aligned rounds
    for p, m in plants:
        seq[p:p + k] = torch.from_numpy(_copy_of(query, k, m)).to(_dev())
    dist = torch.empty(nwin, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    ctx.kmer_hdist_scan_dev(seq, n, k, query, dist)
    ctx.sync()
    planted = [p for p, _ in plants] + [qpos]
    for a, b in [(P32 - 3000, P32 + 3000), (nwin - 4000, nwin)] + [(p - 40, min(p + 40, nwin)) for p in planted]:
        h = seq[a:b + k - 1].cpu().numpy()
        assert np.array_equal(dist[a:b].cpu().numpy(), oracle.kmer_hdist_scan(h, k, query)), (a, b)
    assert [int(dist[p]) for p, _ in plants] == [m for _, m in plants] and int(dist[qpos]) == 0
    return seq, dist, query, planted


def _sparse_hits(ctx, launch, dist, tau, planted):
    """launch(tau, pos, hit_dist, cap, n_hits) on the windows whose distances are `dist`: the list equals nonzero(dist <= tau) with the distances,
    *n_hits its length, the planted positions are in it, nothing is written at or past cap; cap 0 with NULL pointers gives *n_hits alone"""
    import torch
    want = _nonzero_le(dist, tau)
    total = want.numel()
    cap = total + 5
    pos = torch.full((cap + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    hd = torch.full((cap + GUARD,), DIST_FILL, dtype=torch.uint8, device=_dev())
    nh = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    launch(tau, pos, hd, cap, nh)
    ctx.sync()
    assert nh.tolist() == [total, -1], tau
    assert torch.equal(pos[:total], want), tau
    assert torch.equal(hd[:total], dist[want]), tau
    assert bool((pos[total:] == POS_FILL).all()) and bool((hd[total:] == DIST_FILL).all()), "written at or past cap"
    have = set(want.cpu().tolist())
    assert [p for p in planted if p not in have] == [], tau
    nh.fill_(-1)
    torch.cuda.synchronize()
    launch(tau, None, None, 0, nh)
    ctx.sync()
    assert nh.tolist() == [total, -1], tau
    return total


def _dense_hits(ctx, launch, nwin, k, ar):
    """tau = k: every window is a hit.  cap = nwin - 1000 (ranks past 2^32 are written), no distances: pos[r] == r, *n_hits == nwin, nothing at or
    past cap; cap 0 with NULL pointers"""
    import torch
    cap = nwin - 1000
    pos = torch.full((cap + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    nh = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    launch(k, pos, None, cap, nh)
    ctx.sync()
    assert nh.tolist() == [nwin, -1] and nwin > P32
    for i, m in _chunks(cap, ar.numel()):
        assert torch.equal(pos[i:i + m] - i, ar[:m]), i
    assert bool((pos[cap:] == POS_FILL).all()), "written at or past cap"
    del pos
    nh.fill_(-1)
    torch.cuda.synchronize()
    launch(k, None, None, 0, nh)
    ctx.sync()
    assert nh.tolist() == [nwin, -1]


def test_ascii_scan_count_and_hits_past_2_32(ctx, oracle):
    """A: the unaligned scan (+1), the fused counts (aligned: kmer_count3_mfma_kernel, +1: kmer_scan2_kernel) and the hit lists at +0 / +1 / +7
    against the aligned dense scan over the whole 2^32 + 2^20 + 37 bases; the first invalid byte past 2^32 as the count and the hit list report it."""
    import torch
    import bitnuc_amd as bn
    n, k = N_A, K
    nwin = n - k + 1
    _need(11 * n, "2^32-base ASCII scan, counts and hit lists")
    seq, dist, query, planted = _ascii_reference(ctx, oracle)
    # 1. the unaligned scan on the view at +1 byte
    d1 = torch.full((nwin - 1 + GUARD,), DIST_FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    ctx.kmer_hdist_scan_dev(seq.data_ptr() + 1, n - 1, k, query, d1)
    ctx.sync()
    assert _equal(d1[:nwin - 1], dist[1:])
    assert bool((d1[nwin - 1:] == DIST_FILL).all())
    del d1
    # 2. the fused counts, aligned and at +1
    cnt = torch.full((2 + GUARD,), -1, dtype=torch.int64, device=_dev())
    for tau in TAUS:
        want = [_count_le(dist, tau), _count_le(dist[1:], tau)]
        if tau >= k:
            assert want == [nwin, nwin - 1]
        cnt.fill_(-1)
        torch.cuda.synchronize()
        ctx.kmer_hdist_count_dev(seq, n, k, query, tau, cnt)
        ctx.kmer_hdist_count_dev(seq.data_ptr() + 1, n - 1, k, query, tau, cnt.data_ptr() + 8)
        ctx.sync()
        assert cnt[:2].tolist() == want, tau
        assert bool((cnt[2:] == -1).all())
    # 3. the hit lists at +0, +1, +7: sparse (tau 3, 12) and dense (tau = k)
    ar = torch.arange(1 << 27, dtype=torch.int64, device=_dev())
    for o in (0, 1, 7):
        def launch(tau, pos, hd, cap, nh, o=o):
            ctx.kmer_hdist_hits_dev(seq.data_ptr() + o, n - o, k, query, tau, pos, hd, cap, nh)
        for tau in (3, 12):
            _sparse_hits(ctx, launch, dist[o:], tau, [p - o for p in planted])
        _dense_hits(ctx, launch, nwin - o, k, ar)
    del ar
    # 4. the first invalid byte past 2^32 (and a later one), index relative to the pointer passed
    bad = P32 + 3 * 1024 + 77
    seq[bad] = ord("N")
    seq[n - 50] = ord("x")
    pos = torch.full((1024 + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    hd = torch.full((1024 + GUARD,), DIST_FILL, dtype=torch.uint8, device=_dev())
    nh = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    for o in (0, 1):
        torch.cuda.synchronize()
        ctx.kmer_hdist_count_dev(seq.data_ptr() + o, n - o, k, query, 3, cnt)
        with pytest.raises(bn.NucleotideError) as e1:
            ctx.sync()
        want = (e1.value.byte, e1.value.index)
        del e1
        ctx.kmer_hdist_hits_dev(seq.data_ptr() + o, n - o, k, query, 3, pos, hd, 1024, nh)
        with pytest.raises(bn.NucleotideError) as e2:
            ctx.sync()
        assert (e2.value.byte, e2.value.index) == want == (ord("N"), bad - o), o
        del e2
    assert bool((pos[1024:] == POS_FILL).all()) and bool((hd[1024:] == DIST_FILL).all())
    del seq, dist, cnt, pos, hd, nh
    _done("A")


def test_packed_scan_count_and_hits_past_2_32(ctx, oracle):
    """B: the packed scan, count and hit lists on the words of A's sequence, at a 16-byte offset and at 8 mod 16, against the ASCII dense scan."""
    import torch
    n, k = N_A, K
    nwin = n - k + 1
    nw = (n + 31) // 32
    _need(11 * n, "2^32-base packed scan, counts and hit lists")
    seq, dist, query, planted = _ascii_reference(ctx, oracle)
    w16 = torch.empty(nw + 1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.encode_dev(seq, n, w16)
    ctx.sync()
    c0 = P32 // 32 - 100
    assert np.array_equal(w16[c0:c0 + 200].cpu().numpy().view(np.uint64), oracle.encode(seq[32 * c0:32 * (c0 + 200)].cpu().numpy()))
    w8h = torch.zeros(nw + 2, dtype=torch.int64, device=_dev())
    w8h[1:nw + 1] = w16[:nw]
    del seq
    counts = {tau: _count_le(dist, tau) for tau in TAUS}
    ar = torch.arange(1 << 27, dtype=torch.int64, device=_dev())
    cnt = torch.full((1 + GUARD,), -1, dtype=torch.int64, device=_dev())
    for words, align in ((w16[:nw], 0), (w8h[1:nw + 1], 8)):
        assert words.data_ptr() % 16 == align
        dp = torch.full((nwin + GUARD,), DIST_FILL, dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()
        ctx.kmer_hdist_scan_packed_dev(words, nw, n, k, query, dp)
        ctx.sync()
        assert _equal(dp[:nwin], dist), align
        assert bool((dp[nwin:] == DIST_FILL).all())
        del dp
        for tau in TAUS:
            cnt.fill_(-1)
            torch.cuda.synchronize()
            ctx.kmer_hdist_count_packed_dev(words, nw, n, k, query, tau, cnt)
            ctx.sync()
            assert int(cnt[0]) == counts[tau] and (tau < k or counts[tau] == nwin), (align, tau)
            assert bool((cnt[1:] == -1).all())

        def launch(tau, pos, hd, cap, nh, words=words):
            ctx.kmer_hdist_hits_packed_dev(words, nw, n, k, query, tau, pos, hd, cap, nh)
        for tau in (3, 12):
            _sparse_hits(ctx, launch, dist, tau, planted)
        _dense_hits(ctx, launch, nwin, k, ar)
    del dist, w16, w8h, ar, cnt
    _done("B")


def _scan_rounds(n, skip):
    """scan_mfma_host.h: whole rounds of 1024 windows in n bases whose first skip windows are left to the head workgroup"""
    nr = n - skip if n > skip else 0
    return (nr - 32) >> 10 if nr >= 1056 else 0


@pytest.mark.parametrize("woff", (0, 1))
def test_hit_list_scan_of_more_than_2048_tiles(ctx, oracle, woff):
    """C: 2^35 + 2^26 + 19 packed bases, poly-A with exact and near copies of a query that has at least 8 non-A bases (every window that does not
    overlap a copy is more than tau = 3 away): the head windows, both sides of tiles 1023 / 1024 and 2047 / 2048 of the per-trip counts
    (hits_scan_top_kernel carries its sum across chunks of 1024 tiles), window 2^32 - 7, the last whole round and the tail.  Expected list: the
    oracle's scan of each copy's neighbourhood.  Then tau = k (n - k + 1 > 2^35 hits), the packed count, and base counts of the same words."""
    import torch
    n, k, tau = N_C, K, 3
    nwin = n - k + 1
    nw = (n + 31) // 32
    _need(8 * (nw + 2) + (1 << 30), "2^35-base packed hit list")
    rng = np.random.default_rng(2035)
    while True:
        qc = rng.integers(0, 4, size=k)
        if int((qc != 0).sum()) >= 8:
            break
    query = int(sum(int(c) << (2 * i) for i, c in enumerate(qc)))
    # the layout of scan_hits_device.h: counts entry 0 is the head workgroup, 1 + t trip t (windows skip + 4096 t .. + 4095), tile b entries
    # 4096 b .. + 4095; then the tail after the last whole round
    skip = 32 * woff
    rounds = _scan_rounds(n, skip)
    ntiles = ((rounds + 3) // 4 + 2 + 4095) // 4096
    assert 2048 < ntiles < 3072, ntiles  # three chunks of the top scan, the last one partial
    last, tail = skip + 1024 * (rounds - 1), skip + 1024 * rounds
    plants = [(3, 0)]  # the head windows at 8 mod 16 (skip 32), trip 0 at 16
    for b in (1024, 2048):
        wb = skip + 4096 * (4096 * b - 1)  # the first window of counts entry 4096 b: tile b's first
        plants += [(wb - 100, 1), (wb - 15, 0), (wb + 80, 2)]
    plants += [(P32 - 7, 3), (last + 500, 0), (last + 1024 - 10, 1), (tail + 200, 3), (nwin - 1, 2)]
    assert nwin - 1 - tail > 200 + 2 * k
    ps = sorted(p for p, _ in plants)
    assert all(b - a >= 2 * k for a, b in zip(ps, ps[1:]))
    # the planted bases, word by word (the rest is A = 0)
    ascii_words = {}
    for p, m in plants:
        c = _copy_of(query, k, m)
        for i in range(k):
            ascii_words.setdefault((p + i) // 32, np.full(32, ord("A"), dtype=np.uint8))[(p + i) % 32] = c[i]
    widx = sorted(ascii_words)
    wval = np.array([oracle.encode(ascii_words[w][:min(32, n - 32 * w)])[0] for w in widx], dtype=np.uint64)

    def base(j):
        a = ascii_words.get(j // 32)
        return ord("A") if a is None else int(a[j % 32])
    exp_p, exp_d = [], []
    for p, m in sorted(plants):
        a, e = max(0, p - k + 1), min(n, p + 2 * k - 1)
        d = oracle.kmer_hdist_scan(np.array([base(j) for j in range(a, e)], dtype=np.uint8), k, query)
        hit = np.flatnonzero(d <= tau)
        assert a + hit[0] <= p and int(d[p - a]) == m
        exp_p.append(a + hit)
        exp_d.append(d[hit])
    exp_p, exp_d = np.concatenate(exp_p).astype(np.uint64), np.concatenate(exp_d)
    total = exp_p.size
    planted_counts = [sum(int((a[:max(0, min(32, n - 32 * w))] == ord(ch)).sum()) for w, a in ascii_words.items()) for ch in "CGT"]

    buf = torch.zeros(nw + 2, dtype=torch.int64, device=_dev())
    words = buf[woff:woff + nw]
    assert words.data_ptr() % 16 == 8 * woff
    words[torch.tensor(widx, dtype=torch.int64, device=_dev())] = torch.from_numpy(wval.view(np.int64)).to(_dev())
    cap = total + 5
    pos = torch.full((cap + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    hd = torch.full((cap + GUARD,), DIST_FILL, dtype=torch.uint8, device=_dev())
    nh = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    cnt = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_packed_dev(words, nw, n, k, query, tau, pos, hd, cap, nh)
    ctx.kmer_hdist_count_packed_dev(words, nw, n, k, query, tau, cnt)
    ctx.sync()
    assert nh.tolist() == [total, -1] and cnt.tolist() == [total, -1]
    got_p = pos.cpu().numpy().view(np.uint64)
    got_d = hd.cpu().numpy()
    assert np.array_equal(got_p[:total], exp_p), [(int(a), int(b)) for a, b in zip(got_p[:total], exp_p) if a != b][:5]
    assert np.array_equal(got_d[:total], exp_d)
    assert (got_p[total:] == np.uint64(POS_FILL)).all() and (got_d[total:] == DIST_FILL).all()
    # tau = k: every window, ranks far past the small cap are counted but not written
    capd = 1 << 20
    pos = torch.full((capd + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    nh.fill_(-1)
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_packed_dev(words, nw, n, k, query, k, pos, None, capd, nh)
    ctx.sync()
    assert nh.tolist() == [nwin, -1] and nwin > 1 << 35
    assert torch.equal(pos[:capd], torch.arange(capd, dtype=torch.int64, device=_dev()))
    assert bool((pos[capd:] == POS_FILL).all())
    nh.fill_(-1)
    torch.cuda.synchronize()
    ctx.kmer_hdist_hits_packed_dev(words, nw, n, k, query, k, None, None, 0, nh)
    ctx.sync()
    assert nh.tolist() == [nwin, -1]
    # base counts of the same words, then of poly-T
    bc = torch.full((4 + 4,), -1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.base_counts_dev(words, nw, n, bc)
    ctx.sync()
    assert bc[:4].tolist() == [n - sum(planted_counts)] + planted_counts and bc[4:].tolist() == [-1] * 4
    buf.fill_(-1)
    torch.cuda.synchronize()
    ctx.base_counts_dev(words, nw, n, bc)
    ctx.sync()
    assert bc[:4].tolist() == [0, 0, 0, n] and bc[4:].tolist() == [-1] * 4
    del buf, words, pos, hd, nh, cnt, bc
    _done(f"C (words at {8 * woff} mod 16)")


@pytest.mark.parametrize("stride", (1, 2, 4, 16, 5, 12))
def test_window_batches_past_2_32(ctx, oracle, stride):
    """D: as_2bit_batch_dev over every k-mer at stride 1 (kmer_slide2_kernel), 2 / 4 / 16 (kmer_slide_kernel), 5 / 12 (kmer_slide_any_kernel) on
    2^32 + 2^20 + 37 bases: the first / last base of every output against the input, the oracle on the first 2000 outputs, around the first k-mer
    that starts at or past 2^32 and on the last 2000; at strides 1 and 5 an invalid byte past 2^32 reported at its byte offset."""
    import torch
    import bitnuc_amd as bn
    n, k = N_A, K
    count = (n - k) // stride + 1
    _need(n + 8 * (count + GUARD) + (1 << 31), f"stride-{stride} window batch of 2^32 bases")
    seq = torch.empty(n + 16, dtype=torch.uint8, device=_dev())
    ctx.nucgen_dev(seq, n, SEED, flags=2)
    out = torch.full((count + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.as_2bit_batch_dev(seq, k, stride, count, out)
    ctx.sync()
    assert bool((out[count:] == POS_FILL).all()), "written past count"
    for j, m in _chunks(count, 1 << 27):
        o = out[j:j + m]
        first = seq[j * stride:(j + m - 1) * stride + 1:stride]
        lastb = seq[j * stride + k - 1:(j + m - 1) * stride + k:stride]
        assert torch.equal(o & 3, _codes(first).long()) and torch.equal((o >> (2 * k - 2)) & 3, _codes(lastb).long()), (stride, j)
    j0 = -(-P32 // stride)  # the first k-mer whose first base is at or past 2^32
    for a, m in ((0, 2000), (j0 - 1500, 3000), (count - 2000, 2000)):
        h = seq[a * stride:(a + m - 1) * stride + k].cpu().numpy()
        assert np.array_equal(out[a:a + m].cpu().numpy().view(np.uint64), oracle.as_2bit_batch(h, k, stride, m)), (stride, a)
    if stride in (1, 5):
        bad = P32 + 3 * 1024 + 77
        seq[bad] = ord("N")
        torch.cuda.synchronize()
        ctx.as_2bit_batch_dev(seq, k, stride, count, out)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad)
        del ei
    del seq, out
    _done(f"D (stride {stride})")


def test_split_packed_past_2_32(ctx, oracle):
    """E: split_packed_dev of A's words at an odd base past 2^32: canonical == encode of the two ASCII halves; as written: the left words are the
    source's, the right ones the reference's funnel (sampled)."""
    import torch
    n = N_A
    nw = (n + 31) // 32
    idx = P32 + 12347
    _need(3 * n, "split_packed past 2^32")
    seq = torch.empty(n + 16, dtype=torch.uint8, device=_dev())
    ctx.nucgen_dev(seq, n, SEED, flags=2)
    words = torch.empty(nw, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.encode_dev(seq, n, words)
    nl, nr = ctx.split_packed_sizes(nw, n, idx, canonical=True)
    assert (nl, nr) == ((idx + 31) // 32, (n - idx + 31) // 32)
    left = torch.full((nl + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    right = torch.full((nr + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    el, er = torch.empty(nl, dtype=torch.int64, device=_dev()), torch.empty(nr, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.split_packed_dev(words, nw, n, idx, left, right, canonical=True)
    ctx.encode_dev(seq, idx, el)
    ctx.encode_dev(seq.data_ptr() + idx, n - idx, er)  # unaligned device pointer
    ctx.sync()
    assert _equal(left[:nl], el) and _equal(right[:nr], er)
    assert bool((left[nl:] == POS_FILL).all()) and bool((right[nr:] == POS_FILL).all())
    del el, er, left, right
    # as written
    nl, nr = ctx.split_packed_sizes(nw, n, idx)
    assert (nl, nr) == (idx // 32 + 1, nw - idx // 32)
    left = torch.full((nl + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    right = torch.full((nr + GUARD,), POS_FILL, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    ctx.split_packed_dev(words, nw, n, idx, left, right)
    ctx.sync()
    c, s = idx // 32, (idx % 32) * 2
    assert _equal(left[:c], words[:c]) and int(left[c]) & (2**64 - 1) == int(words[c]) & (2**64 - 1) & ((1 << s) - 1)
    for j0 in (0, nr // 2, nr - 1000):
        wh = words[c + j0 - 1 if j0 else c:c + j0 + 1000].cpu().numpy().view(np.uint64)
        wh = np.concatenate([np.zeros(1, np.uint64), wh]) if j0 == 0 else wh
        exp = [(int(wh[j + 1]) >> s) | ((int(wh[j]) << (64 - s)) & (2**64 - 1) if j0 + j else 0) for j in range(1000)]
        assert [int(x) for x in right[j0:j0 + 1000].cpu().numpy().view(np.uint64)] == exp, j0
    assert bool((left[nl:] == POS_FILL).all()) and bool((right[nr:] == POS_FILL).all())
    del seq, words, left, right
    _done("E")
