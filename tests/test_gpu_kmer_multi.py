"""GPU tests of the multi-query k-mer count (bitnuc_kmer_hdist_count_multi*, scan_multi_device.h): counts[q] = windows with distance <= taus[q] to
queries[q], against the oracle's scan per query -- every k, sizes around the round / trip / halo / tail boundaries, query counts around the query block
of 16 and the wave, mixed per-query thresholds, ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte and 8-mod-16
offsets; guard words after the counts; invalid bytes; the n_queries limit; a hipGraph replay after the reference changed; the host forms across the
host chunk; and 10^9 bases with 64 queries against 64 single-query device counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1055, 1056, 1057, 4095, 4127, 4128, 4129, 10**6 + 7)
QS = (1, 2, 31, 32, 33, 64, 257)
GUARD = 8
FILL = 0x5A5A5A5A5A5A5A5A


def _seq(rng, n, k, queries):
    """n ASCII bases, about 30 % lowercase: copies of the queries with a few mutations, then random bases"""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, size=n)
    for i, q in enumerate(queries[:8]):
        p = int(rng.integers(0, max(n - k, 0) + 1)) if n >= k else 0
        qc = np.array([(int(q) >> (2 * b)) & 3 for b in range(k)])
        m = min(k, n - p)
        codes[p:p + m] = qc[:m]
        if i % 2 and m:
            codes[p + int(rng.integers(0, m))] = int(rng.integers(0, 4))
    s = lut[codes]
    s[rng.random(n) < 0.3] |= 0x20
    return s.astype(np.uint8)


def _queries(rng, nq, k):
    """random queries with junk above 2k"""
    q = rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=nq, dtype=np.uint64)
    return q


def _taus(rng, nq, k):
    pool = np.array([0, 1, max(k - 1, 0), k, 2**32 - 1, 2, 3], dtype=np.int64)
    t = pool[np.arange(nq) % pool.size]
    rng.shuffle(t)
    return t.astype(np.uint32)


def _want(oracle, s, k, queries, taus):
    n = s.size
    if n < k:
        return np.zeros(len(queries), dtype=np.uint64)
    return np.array([int(np.count_nonzero(oracle.kmer_hdist_scan(s, k, int(q)) <= int(t))) for q, t in zip(queries, taus)], dtype=np.uint64)


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


def _dev_arrays(queries, taus):
    import torch
    dq = torch.from_numpy(np.asarray(queries, dtype=np.uint64).view(np.int64)).to("cuda:0")
    dt = torch.from_numpy(np.asarray(taus, dtype=np.uint32).view(np.int32)).to("cuda:0")
    counts = torch.full((len(queries) + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    return dq, dt, counts


def _read(ctx, counts, nq):
    ctx.sync()
    c = counts.cpu().numpy().view(np.uint64)
    assert (c[nq:] == np.uint64(FILL)).all(), "counts written after n_queries"
    return c[:nq].copy()


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


def _both(ctx, s, k, queries, taus, off, woff):
    import torch
    n = s.size
    t, ptr = _ascii_dev(s, off)
    w = _pack(s)
    tw, wptr = _words_dev(w, woff)
    assert wptr % 16 == 8 * woff
    dq, dt, c1 = _dev_arrays(queries, taus)
    c2 = torch.full_like(c1, FILL)
    torch.cuda.synchronize()
    ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, len(queries), c1)
    ctx.kmer_hdist_count_multi_packed_dev(wptr, w.size, n, k, dq, dt, len(queries), c2)
    got = _read(ctx, c1, len(queries)), _read(ctx, c2, len(queries))
    del t, tw
    return got


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_size_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(9100 + k)
    for si, n in enumerate(SIZES):
        nq = QS[(si + k) % len(QS)] if n < 10**6 else (33 if k % 2 else 16)
        queries = _queries(rng, nq, k)
        taus = _taus(rng, nq, k)
        s = _seq(rng, n, k, queries)
        want = _want(oracle, s, k, queries, taus)
        a, p = _both(ctx, s, k, queries, taus, (0, 1, 7, 15)[si % 4], si % 2)
        assert np.array_equal(a, want), (n, nq, np.nonzero(a != want)[0][:5])
        assert np.array_equal(p, want), (n, nq, np.nonzero(p != want)[0][:5])


@pytest.mark.parametrize("nq", QS)
def test_query_counts_at_one_size(ctx, oracle, nq):
    rng = np.random.default_rng(500 + nq)
    k, n = 20, 3 * 4096 + 1056 + 77
    queries = _queries(rng, nq, k)
    taus = _taus(rng, nq, k)
    s = _seq(rng, n, k, queries)
    want = _want(oracle, s, k, queries, taus)
    for off in (0, 1, 7, 15):
        a, p = _both(ctx, s, k, queries, taus, off, off & 1)
        assert np.array_equal(a, want) and np.array_equal(p, want), off


def test_mismatch_profile_and_single_count_agree(ctx, oracle):
    """One query repeated with tau 0..3: its mismatch profile in one call; each count equals the single-query device count."""
    import torch
    rng = np.random.default_rng(8)
    k, n = 23, 200_003
    q = int(_queries(rng, 1, k)[0])
    queries = np.array([q] * 4, dtype=np.uint64)
    taus = np.arange(4, dtype=np.uint32)
    s = _seq(rng, n, k, queries)
    want = _want(oracle, s, k, queries, taus)
    assert want[3] > want[0]
    a, p = _both(ctx, s, k, queries, taus, 3, 1)
    assert np.array_equal(a, want) and np.array_equal(p, want)
    t, ptr = _ascii_dev(s, 0)
    one = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for i in range(4):
        ctx.kmer_hdist_count_dev(ptr, n, k, q, i, one)
        ctx.sync()
        assert int(one[0]) == int(want[i])


def test_invalid_byte_and_argument_errors(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(5)
    k, n = 17, 50_000
    queries = _queries(rng, 40, k)
    taus = _taus(rng, 40, k)
    s = _seq(rng, n, k, queries)
    for bad_at, off in ((31_337, 0), (n - 3, 5), (2, 9)):
        b = s.copy()
        b[bad_at] = ord("N")
        b[min(bad_at + 1000, n - 1)] = ord("x")
        t, ptr = _ascii_dev(b, off)
        dq, dt, c = _dev_arrays(queries, taus)
        torch.cuda.synchronize()
        ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, len(queries), c)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing left for the next sync
    dq, dt, c = _dev_arrays(queries, taus)
    t, ptr = _ascii_dev(s, 0)
    torch.cuda.synchronize()
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_count_multi_dev(ptr, n, 33, dq, dt, 40, c)
    assert ei.value.kind == "SequenceTooLong" and ei.value.len == 33
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, 65537, c)
    assert ei.value.kind == "Unsupported"
    with pytest.raises(bn.NucleotideError):
        ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt.data_ptr() + 2, 40, c)
    with pytest.raises(bn.NucleotideError):
        ctx.kmer_hdist_count_multi_packed_dev(dq.data_ptr() + 4, 100, 3000, k, dq, dt, 40, c)
    ctx.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, 0, c)  # nothing to do: nothing written
    ctx.kmer_hdist_count_multi_dev(ptr, k - 1, k, dq, dt, 40, c)  # no windows: zeros
    got = _read(ctx, c, 40)
    assert (got == 0).all()
    del ei


def test_the_query_limit(ctx, oracle):
    """BITNUC_MAX_QUERIES queries in one call (4096 query blocks): a small reference, every count against the host form."""
    rng = np.random.default_rng(65536)
    k, n, nq = 12, 3000, 65536
    queries = _queries(rng, nq, k)
    taus = (np.arange(nq) % 14).astype(np.uint32)
    s = _seq(rng, n, k, queries)
    from bitnuc_amd import api
    want = api.context_free().kmer_hdist_count_multi(s, k, queries[:64], taus[:64])
    assert np.array_equal(want, _want(oracle, s, k, queries[:64], taus[:64]))
    a, p = _both(ctx, s, k, queries, taus, 1, 1)
    # the host form over all of them (windows x queries is above the cutoff: run it on the host form of a free handle in slices)
    free = api.context_free()
    full = np.concatenate([free.kmer_hdist_count_multi(s, k, queries[i:i + 256], taus[i:i + 256]) for i in range(0, nq, 256)])
    assert np.array_equal(a, full) and np.array_equal(p, full)


def test_graph_replay_after_the_reference_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(77)
    n, k, nq = 300_001, 31, 33
    queries = _queries(rng, nq, k)
    taus = _taus(rng, nq, k)
    s1 = _seq(rng, n, k, queries)
    s2 = _seq(rng, n, k, queries)
    want1, want2 = _want(oracle, s1, k, queries, taus), _want(oracle, s2, k, queries, taus)
    assert not np.array_equal(want1, want2)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = _pack(s1)
        tw, wptr = _words_dev(w, 1)
        dq, dt, c1 = _dev_arrays(queries, taus)
        c2 = torch.full_like(c1, FILL)
        c.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, nq, c1)  # warm-up outside the capture: sizes the scratch
        c.kmer_hdist_count_multi_packed_dev(wptr, w.size, n, k, dq, dt, nq, c2)
        assert np.array_equal(_read(c, c1, nq), want1) and np.array_equal(_read(c, c2, nq), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.kmer_hdist_count_multi_dev(ptr, n, k, dq, dt, nq, c1)
                c.kmer_hdist_count_multi_packed_dev(wptr, w.size, n, k, dq, dt, nq, c2)
            t[7:7 + n] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(_pack(s2).view(np.int64)).to(tw.device)
            for _ in range(2):
                c1.fill_(FILL)
                c2.fill_(FILL)
                g.replay()
                assert np.array_equal(_read(c, c1, nq), want2) and np.array_equal(_read(c, c2, nq), want2)
        finally:
            g.reset()
            del g
            c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """Host pointers above the cutoff: chunks of 128 M windows overlapping by k - 1 bases, summed per query; copies of the queries across the boundary."""
    rng = np.random.default_rng(12)
    chunk = 128 << 20
    n, k, nq = chunk + 3_000_000, 25, 5
    queries = _queries(rng, nq, k)
    taus = np.array([0, 2, 5, 25, 2**32 - 1], dtype=np.uint32)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = lut[rng.integers(0, 4, size=n)]
    qb = lut[[(int(queries[0]) >> (2 * i)) & 3 for i in range(k)]]
    for p in (12345, chunk - k - 1, chunk - 3, chunk + k, n - k):
        s[p:p + k] = qb
    want = _want(oracle, s, k, queries, taus)
    assert want[0] >= 5 and want[4] == n - k + 1
    assert np.array_equal(ctx.kmer_hdist_count_multi(s, k, queries, taus), want)
    assert np.array_equal(ctx.kmer_hdist_count_multi_packed(oracle.encode(s), n, k, queries, taus), want)
    import bitnuc_amd as bn
    s[chunk + 99] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.kmer_hdist_count_multi(s, k, queries, taus)
    assert (ei.value.byte, ei.value.index) == (ord("N"), chunk + 99)
    del ei


def test_full_size_64_queries_against_64_single_counts(ctx):
    """10^9 nucgen bases, k = 31, 64 queries (32 taken from known positions, 32 random) with mixed thresholds: the multi-query counts (ASCII and
    packed) against 64 calls of the single-query device count (oracle-checked at this size by test_gpu_fullsize / test_gpu_packed_scan)."""
    import torch
    dev = torch.device("cuda:0")
    n, k, nq = 10**9, 31, 64
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, 0xB17C0DE)
    ctx.sync()
    rng = np.random.default_rng(64)
    queries = []
    for p in rng.integers(0, n - k, size=32):
        h = ref[int(p):int(p) + k].cpu().numpy()
        queries.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
    queries = np.array(queries + [int(x) for x in _queries(rng, 32, k)], dtype=np.uint64)
    taus = np.array([(0, 3, 8, 12, 31, 2**32 - 1, 5, 10)[i % 8] for i in range(nq)], dtype=np.uint32)
    nw = (n + 31) // 32
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    one = torch.zeros(nq, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # torch's fills run on its own stream: done before the context's stream writes these buffers
    ctx.encode_dev(ref, n, words)
    for i in range(nq):
        ctx.kmer_hdist_count_dev(ref, n, k, int(queries[i]), int(taus[i]), one[i:i + 1])
    ctx.sync()
    want = one.cpu().numpy().view(np.uint64).copy()
    assert (want[:32][taus[:32] == 0] >= 1).all()
    dq, dt, c1 = _dev_arrays(queries, taus)
    c2 = torch.full_like(c1, FILL)
    torch.cuda.synchronize()
    ctx.kmer_hdist_count_multi_dev(ref, n, k, dq, dt, nq, c1)
    ctx.kmer_hdist_count_multi_packed_dev(words, nw, n, k, dq, dt, nq, c2)
    assert np.array_equal(_read(ctx, c1, nq), want)
    assert np.array_equal(_read(ctx, c2, nq), want)
