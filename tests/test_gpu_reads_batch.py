"""GPU tests of the best match per read of a ragged batch (bitnuc_reads_hdist_best_batch[_packed]_async, scan_reads_batch_device.h): for every read
behind an offsets table the smallest (distance, query, offset) over all queries and the windows wholly inside the read, against
tests/reads_batch_oracle.py (the oracle library's contiguous scan masked at the reads' ends and reduced per read, or numpy per read) -- every k over
length lists with empty reads, reads below k, reads below a segment, fast-path-only reads, a long read between short ones and boundaries at the round
and trip edges; table spans beyond the wave's slice; matches that straddle two reads (never seen); ties; equality with the fixed-length forms;
invalid bytes; a hipGraph replay after bases, queries and lengths changed; a queue of mixed asynchronous calls; the host forms above the cutoff in
one chunk and across two; argument errors; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases, packed words
at 16-byte and 8-mod-16 offsets with junk pad bits.  Every comparison is exact equality of all three arrays; guard words and bytes surround all
three outputs and best_dist starts at an odd byte offset."""
import numpy as np
import pytest

import reads_batch_oracle as rb
import reads_best_oracle as ro
from test_gpu_reads_best import DOFF, GUARD, Out, _ascii_dev, _dev_queries, _diff, _same, _words_dev

pytestmark = pytest.mark.gpu

QS = (1, 2, 15, 16, 17, 33, 257)
NO = rb.NO_U32
AOFFS = (0, 1, 7, 15)


def _want(oracle, s, off, k, queries):
    """the oracle's contiguous scan, masked and reduced per read (exact); batches without a window: the fill"""
    return rb.batch_best_by_scan(oracle.kmer_hdist_scan, s, off, k, queries)


def _table_dev(t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _both(ctx, s, off, k, queries, aoff=0, woff=0, words=None):
    """((query, pos, dist) of the ASCII form, ... of the packed form); guards checked"""
    import torch
    nq = len(queries)
    count = len(off) - 1
    wo = rb.word_offsets_of(off)
    t, ptr = _ascii_dev(s, aoff)
    w = rb.pack_batch(s, off, seed=k) if words is None else words
    tw, wptr = _words_dev(w, woff)
    d_off, d_wo = _table_dev(off), _table_dev(wo)
    dq = _dev_queries(queries) if nq else None
    o1, o2 = Out(count), Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_best_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs())
    ctx.reads_hdist_best_batch_packed_async(wptr, d_wo, d_off, count, int(wo[-1]), k, dq, nq, *o2.ptrs())
    got = o1.read(ctx), o2.read(ctx)
    del t, tw
    return got


def _check(ctx, oracle, s, off, k, queries, aoff=0, woff=0, words=None, tag=None, want=None):
    want = _want(oracle, s, off, k, queries) if want is None else want
    a, p = _both(ctx, s, off, k, queries, aoff, woff, words)
    assert _same(a, want), ("ascii", tag, k, len(queries), _diff(a, want))
    assert _same(p, want), ("packed", tag, k, len(queries), _diff(p, want))
    return want


# ---- 1. every k, length list, query count and offset -----------------------------------------------------------------------------------
def _length_lists(rng):
    edges = [1023, 1, 1, 3070, 1, 1, 500, 0, 40, 3000, 17, 2100]  # running sums 1023, 1024, 1025, 4095, 4096, 4097: boundaries at round and trip edges
    assert set(np.cumsum(edges)[:6]) == {1023, 1024, 1025, 4095, 4096, 4097}
    return (("short", rng.integers(0, 81, size=3000)),      # empty reads, reads below k, reads below a segment
            ("fast", rng.integers(32, 201, size=2000)),      # fast path only
            ("long", np.array([31, 32, 33, 70_001, 31, 32, 33, 150, 0, 2000])),  # one read walked by several rounds and trips
            ("edges", np.array(edges)))


@pytest.mark.parametrize("k", range(1, 33))
def test_device_forms_every_k_length_list_query_count_and_offset(ctx, oracle, k):
    rng = np.random.default_rng(9300 + k)
    for li, (tag, lengths) in enumerate(_length_lists(rng)):
        nq = QS[(li + k) % len(QS)]
        queries = rb.random_queries(rng, nq, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        _check(ctx, oracle, s, off, k, queries, AOFFS[(li + k) % 4], (li + k // 4) % 2, tag=tag)


# ---- 2. table spans ------------------------------------------------------------------------------------------------------------------------
def _span_lists(rng):
    mid = np.concatenate([rng.integers(40, 300, size=60), np.zeros(200, dtype=np.int64), rng.integers(40, 300, size=60)])
    ends = np.concatenate([np.zeros(7, dtype=np.int64), rng.integers(33, 400, size=80), np.zeros(150, dtype=np.int64)])
    tiny = rng.integers(1, 31, size=4000)  # an ASCII trip of 4096 windows sees more than 132 reads
    one_word = rng.integers(1, 33, size=1500)  # packed: 128 reads per trip ...
    sprinkled = np.where(rng.random(one_word.size * 2) < 0.5, 0, np.repeat(one_word, 2))  # ... and empty reads between them: the span exceeds the slice
    few = np.concatenate([rng.integers(100, 200, size=50), [0, 0, 0], rng.integers(100, 200, size=50), [0], rng.integers(32, 64, size=300)])
    return (("200 empty inside", mid), ("empty at both ends", ends), ("tiny", tiny), ("one word + empties", sprinkled), ("a few empties on the fast path", few))


@pytest.mark.parametrize("k", (1, 12, 31, 32))
def test_table_spans_beyond_and_within_the_slice(ctx, oracle, k):
    rng = np.random.default_rng(2400 + k)
    for li, (tag, lengths) in enumerate(_span_lists(rng)):
        nq = QS[(li + k) % len(QS)]
        queries = rb.random_queries(rng, nq, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        _check(ctx, oracle, s, off, k, queries, AOFFS[(li + k) % 4], li % 2, tag=tag)


def test_a_batch_of_only_empty_reads(ctx):
    off = np.zeros(301, dtype=np.uint64)
    a, p = _both(ctx, np.zeros(0, dtype=np.uint8), off, 5, rb.random_queries(np.random.default_rng(1), 3, 5))
    for got in (a, p):
        assert (got[0] == NO).all() and (got[1] == NO).all() and (got[2] == 0xFF).all()


# ---- 3. windows that straddle two reads ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (20, 32))
@pytest.mark.parametrize("base_len", (33, 150, 1000))
def test_a_match_that_straddles_two_reads_is_not_seen(ctx, oracle, k, base_len):
    """Every split t in 1 .. k - 1: the first t bases of query 0 end read 2 t - 1, the other k - t start read 2 t, on ragged lengths.  The contiguous
    scan finds the copies at distance 0; no read may.  The packed form's pad bits above a read's last base hold the bases that would complete the
    match."""
    rng = np.random.default_rng(2600 + k + base_len)
    count = 2 * k + 1
    lengths = base_len + rng.integers(0, 40, size=count)
    queries = rb.random_queries(rng, 3, k)
    qc = rb.query_codes(queries[0], k)
    off = rb.offsets_of(lengths)
    codes = rng.integers(0, 4, size=int(off[-1]))
    pad = {}
    for t in range(1, k):
        b = int(off[2 * t])  # the boundary between reads 2 t - 1 and 2 t
        codes[b - t:b - t + k] = qc
        pad[2 * t - 1] = list(qc[t:])
    seq = rb.LUT[codes].astype(np.uint8)
    seq[rng.random(seq.size) < 0.3] |= 0x20
    want = _want(oracle, seq, off, k, queries)
    assert (want[2] > 0).all() and (want[2] != 0xFF).all()
    scan = oracle.kmer_hdist_scan(seq, k, int(queries[0]))
    assert sorted(np.nonzero(scan == 0)[0]) == [int(off[2 * t]) - t for t in range(1, k)]
    words = rb.pack_batch(seq, off, pad_codes=pad)
    for aoff, woff in ((0, 0), (7, 1)):
        _check(ctx, oracle, seq, off, k, queries, aoff, woff, words=words, want=want)


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup,nq", ((9, 24), (20, 24), (300, 304)))
def test_ties_the_lowest_query_then_the_lowest_offset(ctx, oracle, dup, nq):
    """The background holds no A and queries 3 and `dup` (the same query block, the next one, a far one) are k A's, every other query starts with A
    and is not all A: only the planted runs of k A's are at distance 0.  Reads 1 .. 4 of 9000 bases hold two runs each, placed so that (ASCII, offset
    0, read r at 9000 r + 50) they fall in two registers of one lane, two lanes of a round, two rounds of a trip and two trips; read 6 holds one run
    in its first segment (where it is B: read 5 ends inside that segment) and one 40 windows later (where it is A).  The lowest query and then the
    lowest offset must win."""
    rng = np.random.default_rng(3500 + dup)
    k = 8
    lengths = [50, 9000, 9000, 9000, 9000, 1007, 300, 0, 77]
    off = rb.offsets_of(lengths)
    codes = rng.integers(1, 4, size=int(off[-1]))
    pairs = {1: (166, 174), 2: (3000, 3100), 3: (500, 500 + 1024), 4: (100, 100 + 4096 + 50), 6: (3, 43)}  # 9050 + 166 = 9216 = 9 * 1024: registers 0 and 4 of lane 0
    for r, (i1, i2) in pairs.items():
        for i in (i1, i2):
            codes[int(off[r]) + i:int(off[r]) + i + k] = 0
    assert int(off[6]) % 32 != 0
    queries = rb.random_queries(rng, nq, k)
    queries &= ~np.uint64(3)  # position 0: A
    queries |= np.uint64(1) << np.uint64(2 * 5)  # position 5: not A
    for q in (3, dup):
        queries[q] &= ~np.uint64((1 << (2 * k)) - 1)  # k A's, junk above 2k kept
    s = rb.LUT[codes].astype(np.uint8)
    want = _want(oracle, s, off, k, queries)
    for r, (i1, _) in pairs.items():
        assert (int(want[0][r]), int(want[1][r]), int(want[2][r])) == (3, i1, 0)
    assert want[2][0] > 0 and want[2][5] > 0 and want[2][7] == 0xFF
    for aoff, woff in ((0, 0), (15, 1)):
        _check(ctx, oracle, s, off, k, queries, aoff, woff, want=want)


# ---- 5. equal lengths: the fixed-length forms' answers, byte for byte ----------------------------------------------------------------------------
@pytest.mark.parametrize("read_len,count", ((31, 3000), (32, 3000), (150, 1500), (1056, 200)))
def test_equal_lengths_equal_the_fixed_length_forms(ctx, read_len, count):
    import torch
    rng = np.random.default_rng(5500 + read_len)
    for k, nq, aoff, woff in ((min(read_len, 32), 17, 1, 1), (13, 33, 0, 0)):
        queries = rb.random_queries(rng, nq, k)
        s = ro.random_reads(rng, read_len, count, k, queries)
        off = rb.offsets_of([read_len] * count)
        words = ro.pack_reads(s, read_len, count)
        a, p = _both(ctx, s, off, k, queries, aoff, woff, words=words)
        t, ptr = _ascii_dev(s, aoff)
        tw, wptr = _words_dev(words, woff)
        dq = _dev_queries(queries)
        o1, o2 = Out(count), Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best_async(ptr, read_len, count, k, dq, nq, *o1.ptrs())
        ctx.reads_hdist_best_packed_async(wptr, read_len, count, k, dq, nq, *o2.ptrs())
        f1, f2 = o1.read(ctx), o2.read(ctx)
        assert _same(a, f1), ("ascii", read_len, k, _diff(a, f1))
        assert _same(p, f2), ("packed", read_len, k, _diff(p, f2))
        assert _same(a, ro.reads_best(s, read_len, count, k, queries) if read_len * count * nq * k < 10**8 else f1)


# ---- 6. invalid bytes ------------------------------------------------------------------------------------------------------------------------
def test_invalid_bytes_are_reported_once_with_the_first_index(ctx, oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(66)
    k, nq = 17, 33
    lengths = rng.integers(0, 300, size=400)
    lengths[200] = 9  # a read shorter than k, in the middle rounds
    queries = rb.random_queries(rng, nq, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    n = int(off[-1])
    count = lengths.size
    want = _want(oracle, s, off, k, queries)
    dq, d_off = _dev_queries(queries), _table_dev(off)
    short_at = int(off[200]) + 4
    for bad_at, second, aoff in ((short_at, n - 10, 0), (n - 1, None, 5), (2, 5000, 9), (31_337, 31_338, 0)):  # inside a short read; the batch's last byte; the head before the first 16-byte boundary; two bad bytes
        b = s.copy()
        b[bad_at] = ord("N")
        if second is not None:
            b[second] = ord("x")
        t, ptr = _ascii_dev(b, aoff)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best_batch_async(ptr, d_off, count, n, k, dq, nq, *o.ptrs())
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing left for the next sync
        t2, ptr2 = _ascii_dev(s, aoff)  # the next call on the same context is clean
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_hdist_best_batch_async(ptr2, d_off, count, n, k, dq, nq, *o.ptrs())
        assert _same(o.read(ctx), want)


# ---- 7. hipGraph -----------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_after_the_bases_the_queries_and_the_lengths_changed(oracle):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    count, k, nq = 2000, 31, 33
    len1 = rng.integers(0, 300, size=count)
    len2 = rng.permutation(len1)  # other lengths, the same count, total bases and total words
    q1, q2 = rb.random_queries(rng, nq, k), rb.random_queries(rng, nq, k)
    (s1, off1), (s2, off2) = rb.random_batch(rng, len1, k, q1), rb.random_batch(rng, len2, k, q2)
    wo1, wo2 = rb.word_offsets_of(off1), rb.word_offsets_of(off2)
    assert off1[-1] == off2[-1] and wo1[-1] == wo2[-1] and not np.array_equal(off1, off2)
    want1, want2 = _want(oracle, s1, off1, k, q1), _want(oracle, s2, off2, k, q2)
    n, nw = int(off1[-1]), int(wo1[-1])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = rb.pack_batch(s1, off1)
        tw, wptr = _words_dev(w, 1)
        dq, d_off, d_wo = _dev_queries(q1), _table_dev(off1), _table_dev(wo1)
        o1, o2 = Out(count), Out(count)
        c.reads_hdist_best_batch_async(ptr, d_off, count, n, k, dq, nq, *o1.ptrs())  # warm-up outside the capture: sizes the scratch
        c.reads_hdist_best_batch_packed_async(wptr, d_wo, d_off, count, nw, k, dq, nq, *o2.ptrs())
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                c.reads_hdist_best_batch_async(ptr, d_off, count, n, k, dq, nq, *o1.ptrs())
                c.reads_hdist_best_batch_packed_async(wptr, d_wo, d_off, count, nw, k, dq, nq, *o2.ptrs())
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(rb.pack_batch(s2, off2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2))
            d_off.copy_(_table_dev(off2))
            d_wo.copy_(_table_dev(wo2))
            for _ in range(2):
                o1.reset()
                o2.reset()
                g.replay()
                assert _same(o1.read(c), want2) and _same(o2.read(c), want2)
        finally:
            g.reset()
            del g
            c.close()


# ---- 8. a queue of mixed asynchronous calls ------------------------------------------------------------------------------------------------
def test_mixed_queue_with_one_sync(ctx, oracle):
    """Both ragged forms between the fixed-length forms, encode_batch_dev and kmer_hdist_best on one context, different (count, n_queries) between
    consecutive calls (the scratch slot's keys and tables are rewritten by each), one sync at the end, every result checked afterwards."""
    import torch
    rng = np.random.default_rng(818)
    k = 21
    dev = torch.device("cuda:0")
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (900, 3))):  # inputs and outputs first
        queries = rb.random_queries(rng, nq, k)
        lengths = np.full(count, 150) if i % 4 >= 2 else rng.integers(0, 260, size=count)
        s, off = rb.random_batch(rng, lengths, k, queries)
        wo = rb.word_offsets_of(off)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, off=off, wo=wo, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         out=Out(count), wdev=_words_dev(rb.pack_batch(s, off), i & 1), d_off=_table_dev(off), d_wo=_table_dev(wo),
                         bpos=torch.zeros(nq, dtype=torch.int64, device=dev), bdist=torch.zeros(nq, dtype=torch.uint8, device=dev),
                         words=torch.zeros(int(wo[-1]) + 1, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    calls = 0
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, s, ptr, dq, o = j["i"], j["count"], j["nq"], j["s"], j["ascii"][1], j["dq"], j["out"].ptrs()
        if i % 4 == 0:
            ctx.reads_hdist_best_batch_async(ptr, j["d_off"], count, s.size, k, dq, nq, *o)
        elif i % 4 == 1:
            ctx.reads_hdist_best_batch_packed_async(j["wdev"][1], j["d_wo"], j["d_off"], count, int(j["wo"][-1]), k, dq, nq, *o)
        elif i % 4 == 2:
            ctx.reads_hdist_best_async(ptr, 150, count, k, dq, nq, *o)
        else:
            ctx.reads_hdist_best_packed_async(j["wdev"][1], 150, count, k, dq, nq, *o)
        if i % 2 == 0:
            ctx.encode_batch_dev(ptr, j["d_off"], j["d_wo"], count, int(j["wo"][-1]), j["words"])
        else:
            ctx.kmer_hdist_best_async(ptr, s.size, k, dq, nq, j["bpos"], j["bdist"])
        calls += 2
    assert calls >= 16
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, s, queries = j["i"], j["s"], j["queries"]
        want = _want(oracle, s, j["off"], k, queries)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        if i % 2 == 0:
            assert np.array_equal(j["words"].cpu().numpy().view(np.uint64)[:-1], rb.pack_batch(s, j["off"], junk=False)), i
        else:
            scans = [oracle.kmer_hdist_scan(s, k, int(q)) for q in queries]
            assert j["bpos"].cpu().tolist() == [int(np.argmin(d)) for d in scans] and j["bdist"].cpu().tolist() == [int(d.min()) for d in scans], i


# ---- 9. the host-pointer forms above the host cutoff -------------------------------------------------------------------------------------------
def test_host_forms_above_the_cutoff_on_a_live_context(oracle):
    """20,000 reads of 0 .. 300 bases and three queries (about 8 * 10^6 window-query pairs, above the default cutoff of 2^20) on a context with the
    default dispatch run through the device in one chunk; a slice below the cutoff and one query passed as a number give the same answers; the table
    errors are the ragged codec's."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(919)
    count, k = 20_000, 23
    lengths = rng.integers(0, 301, size=count)
    queries = rb.random_queries(rng, 3, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    wo = rb.word_offsets_of(off)
    want = _want(oracle, s, off, k, queries)
    words = rb.pack_batch(s, off)
    c = bn.Context(0)
    try:
        assert int(np.maximum(lengths - k + 1, 0).sum()) * 3 >= 1 << 20
        assert _same(c.reads_hdist_best_batch(s, off, k, queries), want)
        assert _same(c.reads_hdist_best_batch_packed(words, wo, off, k, queries), want)
        ew, ewo = c.encode_batch(s, off)  # the recipe: encode_batch, then the packed form
        assert np.array_equal(ewo, wo) and _same(c.reads_hdist_best_batch_packed(ew, ewo, off, k, queries), want)
        one = c.reads_hdist_best_batch(s, off, k, int(queries[1]))  # a scalar query: Q = 1
        assert _same(one, _want(oracle, s, off, k, queries[1:2]))
        m = 1000  # the same call on a slice stays on the host
        assert _same(c.reads_hdist_best_batch(s[:int(off[m])], off[:m + 1], k, queries), tuple(a[:m] for a in want))
        b = s.copy()
        b[s.size - 5] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_hdist_best_batch(b, off, k, queries)
        assert (ei.value.byte, ei.value.index) == (ord("N"), s.size - 5)
        del ei
        assert _same(c.reads_hdist_best_batch(s, off, k, queries), want)  # the next call is clean
        # decreasing offsets are reported exactly as encode_batch does, a foreign word_offsets table as decode_batch does
        dec = off[:6].copy()
        dec[3] = dec[2] - np.uint64(1) if dec[2] else dec[3]
        if dec[3] < dec[2]:
            with pytest.raises(bn.NucleotideError) as e1:
                c.reads_hdist_best_batch(s, dec, k, queries)
            with pytest.raises(bn.NucleotideError) as e2:
                c.encode_batch(s, dec)
            assert (e1.value.kind, e1.value.payload) == (e2.value.kind, e2.value.payload)
            del e1, e2
        wrong = wo[:6].copy()
        wrong[4] += np.uint64(1)
        with pytest.raises(bn.NucleotideError) as e1:
            c.reads_hdist_best_batch_packed(words, wrong, off[:6], k, queries)
        with pytest.raises(bn.NucleotideError) as e2:
            c.decode_batch(words, wrong, off[:6])
        assert (e1.value.kind, e1.value.payload) == (e2.value.kind, e2.value.payload)
        del e1, e2
    finally:
        c.close()


def test_host_forms_across_the_host_chunk(ctx, oracle):
    """900,000 reads of 100 .. 200 bases (about 135 M bases): the ASCII form's first chunk is the longest run of whole reads within 128 Mi bytes, the
    packed form's within 4 Mi words; no read is split, so the reads on both sides of each boundary -- which hold planted copies at their last and
    first windows -- get their own answers.  Then an N past the boundary reports its absolute index."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1292)
    count, k = 900_000, 25
    lengths = rng.integers(100, 201, size=count)
    off = rb.offsets_of(lengths)
    wo = rb.word_offsets_of(off)
    per_ascii = int(np.searchsorted(off, 128 << 20, side="right")) - 1  # the chunk budget: the largest r1 with off[r1] <= 128 Mi
    per_packed = int(np.searchsorted(wo, (128 << 20) // 32, side="right")) - 1
    assert 0 < per_packed < per_ascii < count
    queries = rb.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=int(off[-1]), dtype=np.uint8)
    qc = [rb.query_codes(q, k) for q in queries]
    for per in (per_ascii, per_packed):
        b = int(off[per])
        codes[b - k:b] = qc[0]   # the last window of the chunk's last read
        codes[b:b + k] = qc[1]   # the first window of the next chunk's first read
        b1 = int(off[per + 1])
        codes[b1 + 60:b1 + 60 + k] = qc[0]
    s = rb.LUT[codes]
    del codes
    want = _want(oracle, s, off, k, queries)
    for per in (per_ascii, per_packed):
        assert [tuple(int(a[r]) for a in want) for r in (per - 1, per, per + 1)] == [(0, int(lengths[per - 1]) - k, 0), (1, 0, 0), (0, 60, 0)]
    got = ctx.reads_hdist_best_batch(s, off, k, queries)
    assert _same(got, want), _diff(got, want)
    words, ewo = ctx.encode_batch(s, off)  # (the library's own ragged encoder: zero pad bits)
    assert np.array_equal(ewo, wo)
    got = ctx.reads_hdist_best_batch_packed(words, wo, off, k, queries)
    assert _same(got, want), _diff(got, want)
    bad_at = int(off[per_ascii]) + 99
    s[bad_at] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.reads_hdist_best_batch(s, off, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
    del ei


def test_host_form_validates_a_chunk_that_holds_no_window(ctx):
    """Two reads that fill the ASCII chunk budget of 128 Mi bytes exactly, then a read of 5 bases: the longest run of whole reads within the budget
    ends before it, so it is a chunk of its own with fewer than k bases -- nothing is launched for it, and its bytes are validated all the same (every
    byte of the batch is, whether or not its read can hold a window).  The index is absolute; a clean batch fills the short read."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1301)
    k = 25
    lengths = [(128 << 20) - 1000, 1000, 5]
    off = rb.offsets_of(lengths)
    n = int(off[-1])
    queries = rb.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=n, dtype=np.uint8)
    codes[int(off[2]) - k:int(off[2])] = rb.query_codes(queries[1], k)  # the last window of the first chunk's last read
    s = rb.LUT[codes]
    del codes
    q, p, d = ctx.reads_hdist_best_batch(s, off, k, queries)
    assert (int(q[1]), int(p[1]), int(d[1])) == (1, 1000 - k, 0) and d[0] != 0xFF
    assert (int(q[2]), int(p[2]), int(d[2])) == (int(NO), int(NO), 0xFF)
    s[n - 2] = ord("N")
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.reads_hdist_best_batch(s, off, k, queries)
    assert (ei.value.byte, ei.value.index) == (ord("N"), n - 2)
    del ei
    s[n - 2] = ord("a")
    assert ctx.reads_hdist_best_batch(s, off, k, queries)[2][2] == 0xFF  # the next call is clean


# ---- 10. argument errors, count == 0, no-window calls --------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched_and_no_window_calls_fill(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(12)
    lengths = rng.integers(0, 120, size=100)
    s, off = rb.random_batch(rng, lengths, 12, [])
    wo = rb.word_offsets_of(off)
    n, nw = int(off[-1]), int(wo[-1])
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 1)
    d_off, d_wo = _table_dev(off), _table_dev(wo)
    dq = _dev_queries(np.zeros(16, dtype=np.uint64))
    o = Out(100)
    bq, bp, bd = o.ptrs()
    torch.cuda.synchronize()

    def a_form(seq, table, total, k, q, nq, x, y, z):
        ctx.reads_hdist_best_batch_async(seq, table, 100, total, k, q, nq, x, y, z)

    def p_form(seq, table, total, k, q, nq, x, y, z):
        ctx.reads_hdist_best_batch_packed_async(seq, d_wo if table is d_off else table, d_off, 100, total, k, q, nq, x, y, z)
    for fn, src, total, limit in ((a_form, ptr, n, 2**58), (p_form, wptr, nw, 2**53)):
        for args, kind in (((src, d_off, total, 33, dq, 16, bq, bp, bd), "SequenceTooLong"),       # 2. k > 32
                           ((src, d_off, limit, 12, dq, 65537, bq, bp, bd), "Unsupported"),         # 3. the total, before the query count
                           ((src, d_off, total, 12, dq, 65537, bq, bp, bd), "Unsupported"),         # 4. too many queries
                           ((src, d_off, total, 12, dq, 16, bq, bp + 2, bd), "Unsupported"),        # 6. best_pos not 4-byte aligned
                           ((src, d_off.data_ptr() + 4, total, 12, dq, 16, bq, bp, bd), "Unsupported"),  # 6. a table not 8-byte aligned
                           ((src, None, total, 12, dq, 16, bq, bp, bd), "Unsupported"),             # 6. a table NULL
                           ((None, d_off, total, 12, dq, 16, bq, bp, bd), "Unsupported")):          # 9. the data pointer NULL
            with pytest.raises(bn.NucleotideError) as ei:
                fn(*args)
            assert ei.value.kind == kind, args
            del ei
    # check 3 reports the total, check 4 the query count
    import ctypes as C
    from bitnuc_amd import _lib as L
    lib, err, V = L.load(), L.BitnucErr(), C.c_void_p
    st = lib.bitnuc_reads_hdist_best_batch_async(ctx._h, V(ptr), V(d_off.data_ptr()), 100, 2**58, 12, V(dq.data_ptr()), 65537, V(bq), V(bp), V(bd), C.byref(err))
    assert st == L.UNSUPPORTED and err.value == 2**58
    st = lib.bitnuc_reads_hdist_best_batch_packed_async(ctx._h, V(wptr), V(d_wo.data_ptr()), V(d_off.data_ptr()), 100, 2**53, 12, V(dq.data_ptr()), 65537, V(bq),
                                                        V(bp), V(bd), C.byref(err))
    assert st == L.UNSUPPORTED and err.value == 2**53
    st = lib.bitnuc_reads_hdist_best_batch_async(ctx._h, V(ptr), V(d_off.data_ptr()), 100, n, 12, V(dq.data_ptr()), 65537, V(bq), V(bp), V(bd), C.byref(err))
    assert st == L.UNSUPPORTED and err.value == 65537
    with pytest.raises(bn.NucleotideError):
        ctx.reads_hdist_best_batch_packed_async(wptr + 4, d_wo, d_off, 100, nw, 12, dq, 16, bq, bp, bd)  # 9. words not 8-byte aligned
    ctx.reads_hdist_best_batch_async(ptr, d_off, 0, n, 12, dq, 16, bq, bp, bd)  # count == 0: nothing written, whatever the tables say
    ctx.reads_hdist_best_batch_packed_async(wptr, d_wo, d_off, 0, nw, 12, dq, 16, bq, bp, bd)
    ctx.sync()
    assert o.untouched()
    for k, nq, total_a, total_p in ((0, 16, n, nw), (12, 0, n, nw), (12, 16, 11, 0)):  # k == 0, no queries, total_bases < k / no words: nothing is read (NULL data)
        for call in (lambda: ctx.reads_hdist_best_batch_async(None, d_off, 100, total_a, k, dq if nq else None, nq, bq, bp, bd),
                     lambda: ctx.reads_hdist_best_batch_packed_async(None, d_wo, d_off, 100, total_p, k, dq if nq else None, nq, bq, bp, bd)):
            o.reset()
            torch.cuda.synchronize()
            call()
            q, p, d = o.read(ctx)
            assert (q == NO).all() and (p == NO).all() and (d == 0xFF).all(), (k, nq)
    assert DOFF % 2 == 1 and GUARD > 0


# ---- 11. seeded differential fuzz --------------------------------------------------------------------------------------------------------------
def _fuzz_lengths(rng, count, k):
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return rng.integers(0, 80, size=count)
    if kind == 1:
        return rng.integers(32, 400, size=count)
    if kind == 2:
        return rng.integers(0, k + 2, size=count)  # around k, many without a window
    if kind == 3:
        lens = rng.integers(0, 40, size=count)
        lens[rng.integers(0, count, size=max(1, count // 50))] = rng.integers(2000, 9000, size=max(1, count // 50))
        return lens
    if kind == 4:
        return np.where(rng.random(count) < 0.4, 0, rng.integers(1, 200, size=count))
    return np.full(count, int(rng.integers(1, 200)))


def test_seeded_differential_fuzz(ctx, oracle):
    rng = np.random.default_rng(0xBA7C4)
    for it in range(200):
        k = int(rng.integers(1, 33))
        count = int(rng.integers(1, 3001)) if it % 4 else int(rng.integers(1, 40))
        nq = int(rng.integers(1, 41))
        lengths = _fuzz_lengths(rng, count, k)
        queries = rb.random_queries(rng, nq, k)
        s, off = rb.random_batch(rng, lengths, k, queries)
        want = _want(oracle, s, off, k, queries) if int(off[-1]) >= k else rb.fill(count)
        a, p = _both(ctx, s, off, k, queries, int(rng.integers(0, 16)), int(rng.integers(0, 2)))
        assert _same(a, want), ("ascii", it, k, count, nq, _diff(a, want))
        assert _same(p, want), ("packed", it, k, count, nq, _diff(p, want))
