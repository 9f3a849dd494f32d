"""GPU tests of the sliding k-mer Hamming scan and its fused count on PACKED words (scan_packed_device.h: packed_scan_mfma_kernel,
packed_count3_mfma_kernel) against the oracle's ASCII scan of the decoded sequence: every k, sizes around the round / trip / halo / tail
boundaries, words at 16-byte and 8-mod-16 offsets, distance bytes at odd offsets, the whole tau range, a seeded fuzz, 10^9 bases at k = 31, and the
count captured in a hipGraph."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xB17C0DE
SIZES = (1, 31, 32, 33, 1055, 1056, 1057, 4095, 4096 + 31, 4096 + 32, 4096 + 33, 10**6 + 7)
GUARD = 64


def _words_for(rng, n, k, hits):
    """ceil(n/32) words with junk above 2n; hits: mostly copies of one k-mer (most windows within a small distance), else random bases"""
    nw = (n + 31) // 32
    w = rng.integers(0, 2**64, size=nw, dtype=np.uint64, endpoint=False)
    query = int(rng.integers(0, 2**64, dtype=np.uint64))  # junk above 2k
    if hits and n:
        q = np.array([(query >> (2 * i)) & 3 for i in range(k)], dtype=np.uint64)
        bases = np.resize(q, n)
        flip = rng.random(n) < 0.05
        bases[flip] = rng.integers(0, 4, size=int(flip.sum()), dtype=np.uint64)
        pad = np.zeros(nw * 32, dtype=np.uint64)
        pad[:n] = bases
        sh = (2 * np.arange(32, dtype=np.uint64))
        junk = w[-1]
        w = np.bitwise_or.reduce(pad.reshape(nw, 32) << sh, axis=1)
        if n % 32:
            w[-1] |= junk & ~np.uint64((1 << (2 * (n % 32))) - 1)
    return w.astype(np.uint64), query


def _expect(oracle, words, n, k, query):
    return oracle.kmer_hdist_scan(oracle.decode(words, n), k, query)


def _dev_words(words, off):
    """the words in device memory at an offset of `off` words from a 16-byte aligned allocation"""
    import torch
    t = torch.zeros(words.size + off + 2, dtype=torch.int64, device="cuda:0")
    if words.size:
        t[off:off + words.size] = torch.from_numpy(words.view(np.int64))
    return t, t.data_ptr() + 8 * off


def _run_dev(ctx, oracle, words, n, k, query, woff, doff, taus):
    import torch
    want = _expect(oracle, words, n, k, query)
    nwin = want.size
    t, wp = _dev_words(words, woff)
    assert wp % 16 == 8 * woff
    d = torch.full((nwin + doff + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    cnt = torch.full((len(taus),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()  # the context's stream is not torch's: the buffers are ready before its launches
    ctx.kmer_hdist_scan_packed_dev(wp, words.size, n, k, query, d.data_ptr() + doff)
    for i, tau in enumerate(taus):
        ctx.kmer_hdist_count_packed_dev(wp, words.size, n, k, query, tau, cnt.data_ptr() + 8 * i)
    ctx.sync()
    h = d.cpu().numpy()
    assert np.array_equal(h[doff:doff + nwin], want), (n, k, woff, doff, int(np.nonzero(h[doff:doff + nwin] != want)[0][0]))
    assert (h[:doff] == 0xEE).all() and (h[doff + nwin:] == 0xEE).all(), (n, k, woff, doff)  # nothing written outside the windows
    below = np.cumsum(np.bincount(want, minlength=34)) if nwin else np.zeros(34, dtype=np.int64)
    assert [int(x) for x in cnt.cpu()] == [int(below[min(t, 33)]) for t in taus], (n, k, woff)
    return want


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_and_boundary_size(ctx, oracle, k):
    rng = np.random.default_rng(1000 + k)
    taus = list(range(0, k + 2)) + [2**32 - 1]
    for si, n in enumerate(SIZES):
        for hits in (False, True):
            words, query = _words_for(rng, n, k, hits)
            for woff in (0, 1):
                doff = (0, 1, 3, 15)[(si + 2 * woff + hits) % 4]
                _run_dev(ctx, oracle, words, n, k, query, woff, doff, taus if n < 10**6 or woff == 0 else taus[::4])


def test_device_forms_every_dist_offset(ctx, oracle):
    rng = np.random.default_rng(5)
    for n in (4096 + 33, 10**6 + 7):
        words, query = _words_for(rng, n, 31, True)
        for woff in (0, 1):
            for doff in (0, 1, 3, 15):
                _run_dev(ctx, oracle, words, n, 31, query, woff, doff, [0, 3, 8, 31])


def test_host_pointer_forms_run_the_kernels(ctx, oracle):
    """ctx has force_gpu set: every size goes through the context's scratch and the kernels"""
    rng = np.random.default_rng(11)
    for k in range(1, 33):
        for n in (k, 1057, 4096 + 33, 100_003):
            words, query = _words_for(rng, n, k, k % 2 == 0)
            want = _expect(oracle, words, n, k, query)
            assert np.array_equal(ctx.kmer_hdist_scan_packed(words, n, k, query), want), (k, n)
            for tau in (0, k // 2, k, 2**32 - 1):
                assert ctx.kmer_hdist_count_packed(words, n, k, query, tau) == int((want <= tau).sum()), (k, n, tau)


def test_host_pointer_forms_across_chunks(ctx, oracle):
    """more than one staged chunk (128 Mi windows each, one word of overlap)"""
    rng = np.random.default_rng(12)
    n, k = (1 << 27) + 12_345, 31
    words, query = _words_for(rng, n, k, True)
    want = _expect(oracle, words, n, k, query)
    got = ctx.kmer_hdist_scan_packed(words, n, k, query)
    assert np.array_equal(got, want)
    for tau in (3, 8):
        assert ctx.kmer_hdist_count_packed(words, n, k, query, tau) == int((want <= tau).sum())


def test_seeded_fuzz(ctx, oracle):
    rng = np.random.default_rng(SEED)
    for case in range(300):
        n = int(rng.integers(0, 6000)) if case % 10 else int(rng.integers(6000, 70_000))
        k = int(rng.integers(1, 33))
        words, query = _words_for(rng, n, k, bool(rng.integers(0, 2)))
        woff, doff = int(rng.integers(0, 2)), int(rng.integers(0, 16))
        tau = int(rng.choice([0, int(rng.integers(0, k + 2)), 2**32 - 1]))
        _run_dev(ctx, oracle, words, n, k, query, woff, doff, [tau])


def test_packed_sequence_on_the_device(ctx, oracle):
    from bitnuc_amd import PackedSequence
    rng = np.random.default_rng(3)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=50_001))
    ps = PackedSequence(seq, ctx=ctx)
    query = int(rng.integers(0, 2**62))
    want = oracle.kmer_hdist_scan(seq, 27, query)
    assert np.array_equal(ps.kmer_hdist_scan(27, query), want)
    assert ps.kmer_hdist_count(27, query, 12) == int((want <= 12).sum())


def test_count_captured_in_a_graph_replays(oracle):
    """The count's accumulator and ticket are back at zero after every launch: two replays of a captured count give the right count."""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(21)
    n, k, tau = 3_000_017, 31, 9
    words, query = _words_for(rng, n, k, True)
    want = _expect(oracle, words, n, k, query)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = bn.Context(0, stream=s.cuda_stream)
        t, wp = _dev_words(words, 1)
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        c.kmer_hdist_count_packed_dev(wp, words.size, n, k, query, tau, cnt.data_ptr())  # warm-up outside the capture
        c.sync()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                c.kmer_hdist_count_packed_dev(wp, words.size, n, k, query, tau, cnt.data_ptr() + 8)
            for _ in range(2):
                cnt[1] = -1
                g.replay()
                c.sync()
                assert int(cnt[1]) == int((want <= tau).sum())
            assert int(cnt[0]) == int((want <= tau).sum())
        finally:
            g.reset()
            del g
            c.close()


def test_full_size_every_window_against_the_oracle(ctx, oracle):
    """10^9 bases, k = 31: the words are the oracle's encode of the nucgen stream; all 10^9 - 30 distances by 1 MiB block sums (a block that
    differs is compared in full), and the count at nine thresholds, against the oracle's scan of the same bases."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from bitnuc_amd.dist import scan_shard_range
    dev = torch.device("cuda:0")
    n, k = 10**9, 31
    nwin = n - k + 1
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    ctx.sync()
    h_ref = ref.cpu().numpy()
    del ref
    assert np.array_equal(h_ref[:1 << 20], oracle.nucgen(1 << 20, SEED))
    lib = oracle.lib()
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    nw = (n + 31) // 32
    words = np.zeros(nw, dtype=np.uint64)
    per = (nw + 8 * threads - 1) // (8 * threads)

    def enc(r):
        w0, w1 = r * per, min(nw, (r + 1) * per)
        if w0 >= w1:
            return
        b0, b1 = 32 * w0, min(n, 32 * w1)
        e, cnt = oracle.OrcErr(), C.c_size_t(0)
        assert lib.orc_encode(C.c_void_p(h_ref.ctypes.data + b0), b1 - b0, C.c_void_p(words.ctypes.data + 8 * w0), C.byref(cnt), C.byref(e)) == 0
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(enc, range(8 * threads)))
    qpos = 777_777_777
    q = oracle.as_2bit(h_ref[qpos:qpos + k])
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    dist = torch.empty(nwin, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.kmer_hdist_scan_packed_dev(d_words, nw, n, k, q, dist)
    taus = (0, 8, 16, 20, 23, 26, 30, 31, 40)
    cnt = torch.zeros(len(taus), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for i, tau in enumerate(taus):
        ctx.kmer_hdist_count_packed_dev(d_words, nw, n, k, q, tau, cnt.data_ptr() + 8 * i)
    ctx.sync()
    got_counts = [int(x) for x in cnt.cpu()]
    h_got = dist.cpu().numpy()
    del dist, d_words
    assert int(h_got[qpos]) == 0
    h_exp = np.zeros(nwin, dtype=np.uint8)
    parts = 8 * threads

    def run(r):
        first, count, nread = scan_shard_range(n, k, r, parts)
        if count == 0:
            return 0
        e = oracle.OrcErr()
        st = lib.orc_kmer_hdist_scan(C.c_void_p(h_ref.ctypes.data + first), nread, k, C.c_uint64(q), C.c_void_p(h_exp.ctypes.data + first), C.byref(e))
        assert st == 0, (r, st)
        return count
    with ThreadPoolExecutor(threads) as ex:
        assert sum(ex.map(run, range(parts))) == nwin
    BLK = 1 << 20
    whole = nwin // BLK * BLK
    sums_got = h_got[:whole].view(np.uint64).reshape(-1, BLK // 8).sum(axis=1, dtype=np.uint64)
    sums_exp = h_exp[:whole].view(np.uint64).reshape(-1, BLK // 8).sum(axis=1, dtype=np.uint64)
    badblocks = np.nonzero(sums_got != sums_exp)[0]
    for b in badblocks[:1]:
        i = int(np.nonzero(h_got[b * BLK:(b + 1) * BLK] != h_exp[b * BLK:(b + 1) * BLK])[0][0]) + int(b) * BLK
        raise AssertionError(f"window {i}: kernel {h_got[i]}, oracle {h_exp[i]} ({len(badblocks)} of {whole // BLK} blocks differ)")
    assert np.array_equal(h_got[whole:], h_exp[whole:])
    below = np.cumsum(np.bincount(h_exp, minlength=k + 1))
    assert got_counts == [int(below[min(t, k)]) for t in taus], (got_counts, [int(below[min(t, k)]) for t in taus])
    assert got_counts[-1] == nwin
