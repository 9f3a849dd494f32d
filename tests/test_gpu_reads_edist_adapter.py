"""GPU tests of the 3' adapter per read (bitnuc_reads_edist_adapter[_packed]_async, _adapter_batch[_packed]_async, the pattern twins and the host forms
above the cutoff; reads_edist_adapter_kernel, scan_edist_adapter_device.h) against tests/reads_edist_adapter_oracle.py (the plain DP over all rows, the cut a
direct Levenshtein minimum).  One read per lane; the whole-read walk in pieces of 64 bases, then the decode of the last column into the overhang candidates,
then one backward walk per read for the cut; the ragged layout's masked loop snapshots the column at a lane's own last base.  So: counts around the wave and
the block and one beyond the bounded grid; lengths around the pieces; one read of 70,000 bases whose only admissible candidate is an overhang at its end;
waves of 64 different lengths (0 and lengths below k included), of equal lengths and without a read of k bases; k in {1, 2, 16, 31, 32}; min_overlap in
{1, 3, k}; rates 0/1, 1/10, 1/5, 1/1; Q around the interleave factor and at the limit; the planted reads of tests/reads_edist_adapter_cases.py on both
layouts; reads that end at the last byte or word of their allocation; invalid bytes at a piece's first and last byte; a hipGraph replay after lengths, reads
and queries changed; a queue mixed with reads_edist_best_async and reads_edist_start_async; the host forms in one chunk and across two; the bitnuc.hpp
methods; the header's six identities; a seeded differential fuzz.  ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte
and 8-mod-16 offsets with junk pad bits run on the same data.  Every comparison is exact equality of all five arrays; guard words and bytes surround the
outputs and both byte arrays start at odd offsets."""
import numpy as np
import pytest

import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_adapter_cases as cases
import reads_edist_adapter_oracle as ao
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
OFFS = (0, 1, 7, 15)
RATES = [(0, 1), (1, 10), (1, 5), (1, 1)]
MAX_QUERIES = 65536


def _rule(i, k):
    """the i-th (min_overlap, err_num, err_den) of a rotation over min_overlap in {1, 3, k} and the four rates"""
    return (sorted({1, min(3, k), k})[i % len({1, min(3, k), k})],) + RATES[(i // 3 + i) % 4]


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _dev_queries(queries, pattern=False):
    import torch
    if pattern:
        return torch.from_numpy(rp.as_patterns(queries).view(np.int32).copy()).to("cuda:0")
    return _dev_u64(np.asarray(queries, dtype=np.uint64).reshape(-1))


class Out:
    """adapter / cut / end with GUARD words before and after [0, count); overlap / dist inside guarded buffers, starting at odd bytes"""

    def __init__(self, count):
        import torch
        self.count = count
        self.w = [torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        self.d = [torch.full((off + count + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0") for off in DOFFS]

    def ptrs(self):
        return [a.data_ptr() + 4 * GUARD for a in self.w] + [d.data_ptr() + off for d, off in zip(self.d, DOFFS)]

    def reset(self):
        for a in self.w:
            a.fill_(FILL32)
        for a in self.d:
            a.fill_(0x5A)

    def untouched(self):
        return all(bool((a == FILL32).all()) for a in self.w) and all(bool((a == 0x5A).all()) for a in self.d)

    def read(self, ctx=None):
        if ctx is not None:
            ctx.sync()
        n = self.count
        out = []
        for a in self.w:
            a = a.cpu().numpy().view(np.uint32)
            assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "adapter / cut / end written outside [0, count)"
            out.append(a[GUARD:GUARD + n].copy())
        for d, off in zip(self.d, DOFFS):
            d = d.cpu().numpy()
            assert (d[:off] == 0x5A).all() and (d[off + n:] == 0x5A).all(), "overlap / dist written outside [0, count)"
            out.append(d[off:off + n].copy())
        return tuple(out)


def _ascii_dev(s, off, tail=16):
    """s at byte offset `off` of a device buffer; the bytes around it are zeros: invalid, must never be examined.  tail = 0: the batch ends with the buffer"""
    import torch
    t = torch.zeros(s.size + off + tail, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    return t, t.data_ptr() + off


def _words_dev(w, off, tail=2):
    import torch
    t = torch.zeros(w.size + off + tail, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero(np.any([g != w for g, w in zip(got, want)], axis=0))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


def _fns(ctx, pattern, ragged):
    name = "reads_" + ("pattern_" if pattern else "") + "edist_adapter" + ("_batch" if ragged else "")
    return getattr(ctx, name + "_async"), getattr(ctx, name + "_packed_async")


def _ragged(ctx, s, off, k, queries, rule, aoff=0, woff=0, pattern=False, tail=True):
    """(the outputs of the ragged ASCII form, of the ragged packed form), guards checked"""
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count, nq = off.size - 1, len(queries)
    wtab = rb.word_offsets_of(off)
    w = rb.pack_batch(s, off, seed=k)
    t, ptr = _ascii_dev(s, aoff, 16 if tail else 0)
    tw, wptr = _words_dev(w, woff, 2 if tail else 0)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_queries(queries, pattern)
    o1, o2 = Out(count), Out(count)
    fa, fp = _fns(ctx, pattern, True)
    torch.cuda.synchronize()
    fa(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs(), *rule)
    fp(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o2.ptrs(), *rule)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _fixed(ctx, s, n, count, k, queries, rule, aoff=0, woff=0, pattern=False, tail=True):
    import torch
    nq = len(queries)
    w = ro.pack_reads(s, n, count)
    t, ptr = _ascii_dev(s[:n * count], aoff, 16 if tail else 0)
    tw, wptr = _words_dev(w, woff, 2 if tail else 0)
    dq = _dev_queries(queries, pattern)
    o1, o2 = Out(count), Out(count)
    fa, fp = _fns(ctx, pattern, False)
    torch.cuda.synchronize()
    fa(ptr, n, count, k, dq, nq, *o1.ptrs(), *rule)
    fp(wptr, n, count, k, dq, nq, *o2.ptrs(), *rule)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check_ragged(ctx, s, off, k, queries, rule, want=None, tag=(), pattern=False, **kw):
    if want is None:
        want = (ao.reads_pattern_edist_adapter_batch if pattern else ao.reads_edist_adapter_batch)(s, off, k, queries, *rule)
    a, p = _ragged(ctx, s, off, k, queries, rule, pattern=pattern, **kw)
    assert _same(a, want), ("ragged ascii", tag, rule, _diff(a, want))
    assert _same(p, want), ("ragged packed", tag, rule, _diff(p, want))
    return want


def _check_fixed(ctx, s, n, count, k, queries, rule, want=None, tag=(), pattern=False, **kw):
    if want is None:
        want = (ao.reads_pattern_edist_adapter if pattern else ao.reads_edist_adapter)(s, n, count, k, queries, *rule)
    a, p = _fixed(ctx, s, n, count, k, queries, rule, pattern=pattern, **kw)
    assert _same(a, want), ("fixed ascii", tag, rule, _diff(a, want))
    assert _same(p, want), ("fixed packed", tag, rule, _diff(p, want))
    return want


def _check_both(ctx, s, n, count, k, queries, rule, tag=(), i=0, **kw):
    """equal lengths: the fixed and the ragged layout on the same data (identity 4; the ASCII and the packed form agree: identity 6)"""
    want = _check_fixed(ctx, s, n, count, k, queries, rule, tag=tag, aoff=OFFS[i % 4], woff=i % 2, **kw)
    _check_ragged(ctx, s, rb.offsets_of([n] * count), k, queries, rule, want=want, tag=tag, aoff=OFFS[(i + 1) % 4], woff=(i + 1) % 2, **kw)
    return want


def _wave_lengths(rng, count, k, top=150):
    """waves of 64 consecutive reads with 64 different lengths each: 0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 150 and others up to `top`"""
    out = []
    must = sorted({0, max(k - 1, 0), k, k + 1, 63, 64, 65, 127, 128, 129, 150})
    while len(out) < count:
        rest = [x for x in rng.permutation(top + 1) if x not in must][:64 - len(must)]
        wave = must + [int(x) for x in rest]
        rng.shuffle(wave)
        out += wave
    return out[:count]


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_counts_around_the_wave_and_the_block(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, nq) in enumerate(((16, 9), (31, 3), (2, 5))):
        queries, s, off = cases.random_reads(rng, _wave_lengths(rng, count, k), k, nq)
        _check_ragged(ctx, s, off, k, queries, _rule(i + count, k), aoff=OFFS[(i + count) % 4], woff=(i + count) % 2, tag=(count, k))
        n = (65, 150, 64)[i]
        queries, s, off = cases.random_reads(rng, [n] * count, k, nq)
        _check_both(ctx, s, n, count, k, queries, _rule(i + count + 1, k), tag=(count, k, n), i=i + count)


def test_a_count_beyond_the_bounded_grid(ctx):
    """one read more than the grid has lanes (8 workgroups of 256 lanes per CU): one lane walks two reads; reads of k bases (the oracle works each of the
    4^6 different reads out once)"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 1
    rng = np.random.default_rng(5)
    k, nq = 6, 3
    queries = ro.random_queries(rng, nq, k)
    s = ro.LUT[rng.integers(0, 4, size=count * k)].astype(np.uint8)
    want = _check_fixed(ctx, s, k, count, k, queries, (3, 1, 5), aoff=1, woff=1)
    assert (want[0] != ao.NO_U32).any() and (want[3][want[0] != ao.NO_U32] < k).any()
    lengths = np.full(count, k)
    lengths[-1], lengths[0] = k - 1, k + 1  # (the same total: a ragged batch whose last read, the second of lane 0, is too short)
    _check_ragged(ctx, s, rb.offsets_of(lengths), k, queries, (3, 1, 5), aoff=7, woff=0)


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_lengths_around_the_pieces_on_both_layouts(ctx, k):
    rng = np.random.default_rng(200 + k)
    for i, n in enumerate((k, k + 1, 63, 64, 65, 127, 128, 129, 150)):
        if n < k:
            continue
        queries, s, off = cases.random_reads(rng, [n] * 70, k, 5)
        _check_both(ctx, s, n, 70, k, queries, _rule(i, k), tag=(k, n), i=i)


def test_one_read_of_70000_bases_whose_only_admissible_candidate_is_an_overhang_at_its_end(ctx):
    rng = np.random.default_rng(31)
    k, n = 16, 70_000
    q16 = np.array([0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 1, 3])  # ACGTAACCGGTTAGCT
    far = np.array([3] * 15 + [1])
    codes = np.full(n, 2, dtype=np.int64)  # a run of G: no adapter aligns with it within the rate
    codes[n - 11:] = q16[:11]
    s = ro.LUT[codes].astype(np.uint8)
    queries = np.array([ro.word_of(far), ro.word_of(q16), ro.word_of(far[::-1])], dtype=np.uint64)
    rule = (3, 1, 10)
    want = ao.reads_edist_adapter(s, n, 1, k, queries, *rule)
    assert tuple(int(a[0]) for a in want) == (1, n - 11, n, 11, 0)
    _check_fixed(ctx, s, n, 1, k, queries, rule, want=want, aoff=1, woff=1)
    # ragged: the long read in a wave of short ones (the masked loop runs 70,000 steps for every lane; each lane keeps the column of ITS last base)
    lengths = [100, n, 15, 0, 185]
    q2, short, soff = cases.random_reads(rng, [100, 15, 0, 185], k, 3)
    b = np.concatenate([short[:100], s, short[100:]])
    w = ao.reads_edist_adapter_batch(short, soff, k, queries, *rule)
    w = tuple(np.concatenate([a[:1], x, a[1:]]) for a, x in zip(w, want))
    _check_ragged(ctx, b, rb.offsets_of(lengths), k, queries, rule, want=w, aoff=7, woff=0)


@pytest.mark.parametrize("k", [1, 16, 32])
def test_ragged_waves_all_different_all_equal_and_without_a_read_of_k_bases(ctx, k):
    rng = np.random.default_rng(300 + k)
    lengths = _wave_lengths(rng, 64, k)                                  # wave 0: 64 different lengths
    lengths += [130] * 64                                                # wave 1: equal lengths, the unmasked loop
    lengths += [int(x) for x in rng.integers(0, k, size=64)]             # wave 2: no read of k bases
    lengths += [k] * 64                                                  # wave 3: equal, one piece
    lengths += _wave_lengths(rng, 40, k, top=300)
    queries, s, off = cases.random_reads(rng, lengths, k, 7)
    for i in range(2):
        want = _check_ragged(ctx, s, off, k, queries, _rule(i + k, k), aoff=15, woff=1)
        assert (want[3][128:192] == 255).all()


@pytest.mark.parametrize("k", [2, 16, 31])
def test_every_overlap_rule_and_rate(ctx, k):
    rng = np.random.default_rng(350 + k)
    queries, s, off = cases.random_reads(rng, _wave_lengths(rng, 130, k), k, 6)
    qf, f, _ = cases.random_reads(rng, [97] * 130, k, 6)
    i = 0
    for mo in sorted({1, min(3, k), k}):
        for num, den in RATES:
            _check_ragged(ctx, s, off, k, queries, (mo, num, den), aoff=OFFS[i % 4], woff=i % 2)
            _check_fixed(ctx, f, 97, 130, k, qf, (mo, num, den), aoff=OFFS[(i + 2) % 4], woff=(i + 1) % 2)
            i += 1


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 9, 17])
def test_queries_around_the_interleave_factor(ctx, nq):
    rng = np.random.default_rng(400 + nq)
    k = 16
    queries, s, off = cases.random_reads(rng, _wave_lengths(rng, 96, k), k, nq)
    _check_ragged(ctx, s, off, k, queries, _rule(nq, k), aoff=OFFS[nq % 4], woff=nq % 2)
    queries, s, off = cases.random_reads(rng, [129] * 66, k, nq)
    _check_both(ctx, s, 129, 66, k, queries, _rule(nq + 1, k), i=nq)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES adapters, few reads: the reads carry prefixes of the LAST adapters, and of adapter 0 for the tie towards the lower index"""
    rng = np.random.default_rng(41)
    k, n, count = 16, 20, 5
    queries = rng.permutation(np.arange(1 << 20, dtype=np.uint64))[:MAX_QUERIES] * np.uint64(4099)  # distinct 2-bit words
    s = ro.LUT[rng.integers(0, 4, count * n)].astype(np.uint8)
    for r, q in enumerate((MAX_QUERIES - 1, 0, MAX_QUERIES - 2, 12345)):
        s[r * n + n - 13:(r + 1) * n] = ro.LUT[np.asarray(ro.query_codes(queries[q], k), dtype=np.int64)[:13]]
    want = _check_fixed(ctx, s, n, count, k, queries, (12, 0, 1), aoff=7, woff=1)
    assert [int(x) for x in want[0][:4]] == [MAX_QUERIES - 1, 0, MAX_QUERIES - 2, 12345] and (want[3][:4] == 13).all()
    _check_ragged(ctx, s, rb.offsets_of([n] * count), k, queries, (12, 0, 1), want=want)


def test_ascii_and_packed_offsets_on_the_same_data_and_reads_that_end_with_their_allocation(ctx):
    rng = np.random.default_rng(43)
    k = 31
    lengths = _wave_lengths(rng, 100, k)
    lengths[-1] = 129  # the last read has bases: the batch's last byte and word are its own
    queries, s, off = cases.random_reads(rng, lengths, k, 5)
    assert (s & 0x20).any()
    rule = (3, 1, 10)
    want = ao.reads_edist_adapter_batch(s, off, k, queries, *rule)
    qf, f, _ = cases.random_reads(rng, [65] * 67, k, 5)
    wantf = ao.reads_edist_adapter(f, 65, 67, k, qf, *rule)
    for i, aoff in enumerate(OFFS):
        _check_ragged(ctx, s, off, k, queries, rule, want=want, aoff=aoff, woff=i % 2, tail=i % 2 == 0)
        _check_fixed(ctx, f, 65, 67, k, qf, rule, want=wantf, aoff=aoff, woff=(i + 1) % 2, tail=i % 2 == 1)


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_planted_reads_by_hand_on_both_layouts(ctx, case):
    name, reads, adapters, mo, num, den, want = case
    s, queries = cases.arrays(reads, adapters)
    want = cases.want_arrays(want)
    _check_both(ctx, s, cases.N, len(reads), cases.K, queries, (mo, num, den), i=len(name))
    a, p = _fixed(ctx, s, cases.N, len(reads), cases.K, queries, (mo, num, den), aoff=7)
    assert _same(a, want) and _same(p, want), (_diff(a, want), _diff(p, want))
    # in a wave of other lengths: the masked loop and its snapshot
    rng = np.random.default_rng(len(name))
    _, pad, _ = cases.random_reads(rng, [47, 0, 101], cases.K, 1, share=0)
    pad = np.frombuffer(bytes(pad).upper().replace(b"A", b"C").replace(b"G", b"T"), dtype=np.uint8)
    b = np.concatenate([pad[:47], s, pad[47:]])
    off = rb.offsets_of([47, 0] + [cases.N] * len(reads) + [101])
    a, p = _ragged(ctx, b, off, cases.K, queries, (mo, num, den), aoff=1, woff=1)
    assert _same(tuple(x[2:-1] for x in a), want) and _same(tuple(x[2:-1] for x in p), want), (_diff(tuple(x[2:-1] for x in a), want))


# ---- 2. validation, errors, graphs, queues, host forms ------------------------------------------------------------------------------------

def test_invalid_bytes_at_a_pieces_first_and_last_byte_and_in_a_read_shorter_than_k(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, nq = 17, 9
    lengths = [150, 16, 200, 0, 3, 129, 64, 16]
    queries, s, off = cases.random_reads(rng, lengths, k, nq)
    o_ = [int(x) for x in off]
    count = len(lengths)
    rule = (3, 1, 10)
    want = ao.reads_edist_adapter_batch(s, off, k, queries, *rule)
    dq, d_off = _dev_queries(queries), _dev_u64(off)
    b = s.copy()
    for r in (1, 4, 7):
        b[o_[r]:o_[r + 1]] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=lengths[r])  # every byte of the reads shorter than k
    for aoff in (0, 3):
        t, ptr = _ascii_dev(b, aoff)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_adapter_batch_async(ptr, d_off, count, o_[-1], k, dq, nq, *o.ptrs(), *rule)
        assert _same(o.read(ctx), want)  # no error, correct results
    # a piece's first byte (base 64 of read 2), a piece's last byte (base 127 of read 5), a read's last byte (read 6, base 63), the batch's first byte
    for bad_at, later, aoff in ((o_[2] + 64, o_[5] + 5, 0), (o_[5] + 127, o_[6] + 1, 9), (o_[6] + 63, None, 5), (0, o_[2] + 128, 1)):
        c = b.copy()
        c[bad_at] = ord("N")
        if later is not None:
            c[later] = ord("x")  # a later one: the first in buffer order wins
        t, ptr = _ascii_dev(c, aoff)
        o = Out(count)
        torch.cuda.synchronize()
        ctx.reads_edist_adapter_batch_async(ptr, d_off, count, o_[-1], k, dq, nq, *o.ptrs(), *rule)
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.sync()
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
        ctx.sync()  # latched once: nothing is left for the next sync
    # the fixed layout: reads of 129 bases, an N at the last byte of the last read and an earlier one at a piece's first byte
    n, cnt = 129, 5
    q2, f, _ = cases.random_reads(rng, [n] * cnt, k, nq)
    f[4 * n + 128] = ord("N")
    f[2 * n + 64] = ord("n")
    t, ptr = _ascii_dev(f, 7)
    o = Out(cnt)
    torch.cuda.synchronize()
    ctx.reads_edist_adapter_async(ptr, n, cnt, k, _dev_queries(q2), nq, *o.ptrs(), *rule)
    with pytest.raises(bn.NucleotideError) as ei:
        ctx.sync()
    assert (ei.value.byte, ei.value.index) == (ord("n"), 2 * n + 64)
    del ei
    t2, ptr2 = _ascii_dev(b, 1)  # the next call on the same context is clean and correct
    o = Out(count)
    torch.cuda.synchronize()
    ctx.reads_edist_adapter_batch_async(ptr2, d_off, count, o_[-1], k, dq, nq, *o.ptrs(), *rule)
    assert _same(o.read(ctx), want)


def test_argument_errors_and_fills_on_the_device(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(8)
    k, n, count = 16, 60, 9
    queries, s, off = cases.random_reads(rng, [n] * count, k, 3)
    t, ptr = _ascii_dev(s, 0)
    dq = _dev_queries(queries)
    o = Out(count)
    torch.cuda.synchronize()
    for kw, value in ((dict(min_overlap=0), 0), (dict(min_overlap=17), 17), (dict(err_den=0, err_num=4), 4), (dict(err_num=11), 11)):
        with pytest.raises(bn.NucleotideError) as ei:
            ctx.reads_edist_adapter_async(ptr, n, count, k, dq, 3, *o.ptrs(), **kw)
        assert ei.value.kind == "Unsupported", (kw, value)  # (the reported value: tests/test_reads_edist_adapter_host.py)
        del ei
    for bad in range(5):
        p = o.ptrs()
        p[bad] = 0
        with pytest.raises(bn.NucleotideError):
            ctx.reads_edist_adapter_async(ptr, n, count, k, dq, 3, *p)
    with pytest.raises(bn.NucleotideError):
        ctx.reads_edist_adapter_async(ptr, n, count, 33, dq, 3, *o.ptrs())
    ctx.sync()
    assert o.untouched()
    for args in ((n, count, 0, dq, 3), (n, count, k, dq, 0), (k - 1, count, k, dq, 3)):  # k == 0, no queries, read_len < k: the fill, nothing read
        o.reset()
        ctx.reads_edist_adapter_async(0, *args, *o.ptrs())
        assert _same(o.read(ctx), ao.fill5(count)), args[:3]


def test_graph_replay_after_the_lengths_the_reads_and_the_queries_changed():
    """the tables are read on the device at every replay: the same count and totals, other lengths, reads and queries give the new answers"""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    k, nq, count = 31, 9, 640
    rule = (3, 1, 10)
    l1 = np.array(_wave_lengths(rng, count, k))
    l1[(l1 % 32 == 0) & (l1 > 0)] += 1  # no multiple of 32: a permutation then keeps the words' total as well
    l2 = rng.permutation(l1)
    (q1, s1, off1), (q2, s2, off2) = cases.random_reads(rng, l1, k, nq), cases.random_reads(rng, l2, k, nq)
    w1tab, w2tab = rb.word_offsets_of(off1), rb.word_offsets_of(off2)
    assert int(off1[-1]) == int(off2[-1]) and int(w1tab[-1]) == int(w2tab[-1]) and not np.array_equal(off1, off2)
    want1, want2 = ao.reads_edist_adapter_batch(s1, off1, k, q1, *rule), ao.reads_edist_adapter_batch(s2, off2, k, q2, *rule)
    n = 129
    _, f1, _ = cases.random_reads(rng, [n] * 100, k, nq)
    _, f2, _ = cases.random_reads(rng, [n] * 100, k, nq)
    f2[50 * n + n - 20:51 * n] = ro.LUT[np.asarray(ro.query_codes(q2[3], k), dtype=np.int64)[:20]]
    wantf1, wantf2 = ao.reads_edist_adapter(f1, n, 100, k, q1, *rule), ao.reads_edist_adapter(f2, n, 100, k, q2, *rule)
    assert tuple(int(a[50]) for a in wantf2) == (3, n - 20, n, 20, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = rb.pack_batch(s1, off1)
        tw, wptr = _words_dev(w, 1)
        tf, fptr = _ascii_dev(f1, 1)
        dq, d_off, d_wtab = _dev_queries(q1), _dev_u64(off1), _dev_u64(w1tab)
        o1, o2, o3 = Out(count), Out(count), Out(100)

        def run():
            c.reads_edist_adapter_batch_async(ptr, d_off, count, int(off1[-1]), k, dq, nq, *o1.ptrs(), *rule)
            c.reads_edist_adapter_batch_packed_async(wptr, d_wtab, d_off, count, int(w1tab[-1]), k, dq, nq, *o2.ptrs(), *rule)
            c.reads_edist_adapter_async(fptr, n, 100, k, dq, nq, *o3.ptrs(), *rule)
        run()  # warm-up outside the capture: sizes the scratch
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1) and _same(o3.read(c), wantf1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                run()
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(rb.pack_batch(s2, off2).view(np.int64)).to(tw.device)
            tf[1:1 + f2.size] = torch.from_numpy(f2).to(tf.device)
            dq.copy_(_dev_queries(q2))
            d_off.copy_(_dev_u64(off2))
            d_wtab.copy_(_dev_u64(w2tab))
            o1.reset(), o2.reset(), o3.reset()
            g.replay()
            assert _same(o1.read(c), want2) and _same(o2.read(c), want2) and _same(o3.read(c), wantf2)
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_with_reads_edist_best_and_reads_edist_start(ctx):
    """all eight _async forms in turn between reads_edist_best_async and reads_edist_start_async calls on one context (they share the table slot in stream
    order), different (count, n_queries) between consecutive calls, one sync at the end, every result checked afterwards.  With min_overlap = k and rate 1/1
    the adapter call IS the pair: (adapter, end, dist) the best triple, (cut, dist) the start stage's answer on it (identity 1)"""
    import torch
    rng = np.random.default_rng(809)
    k, n = 21, 75
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (700, 1), (333, 17), (90, 40), (600, 16), (7, 2), (300, 3))):
        ragged = i % 2 == 1
        lengths = rng.integers(0, 150, size=count) if ragged else np.full(count, n)
        queries, s, off = cases.random_reads(rng, lengths, k, nq)
        wtab = rb.word_offsets_of(off)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, off=off, wtab=wtab, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         dp=_dev_queries(rp.singletons(queries, k), True), d_off=_dev_u64(off), d_wtab=_dev_u64(wtab), out=Out(count), full=Out(count),
                         best=Out(count), start=Out(count), wdev=_words_dev(rb.pack_batch(s, off), i & 1), ragged=ragged, rule=_rule(i, k)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, ptr, dq, dp = j["i"], j["count"], j["nq"], j["ascii"][1], j["dq"], j["dp"]
        total, wtotal, wptr = int(j["off"][-1]), int(j["wtab"][-1]), j["wdev"][1]
        form = i // 2 % 4
        bq, _, be, _, bd = j["best"].ptrs()
        _, st, _, _, sd = j["start"].ptrs()
        if j["ragged"]:
            heads = [(ptr, j["d_off"], count, total), (wptr, j["d_wtab"], j["d_off"], count, wtotal)]
            fn = [ctx.reads_edist_adapter_batch_async, ctx.reads_edist_adapter_batch_packed_async, ctx.reads_pattern_edist_adapter_batch_async,
                  ctx.reads_pattern_edist_adapter_batch_packed_async][form]
            fn(*heads[form % 2], k, dp if form >= 2 else dq, nq, *j["out"].ptrs(), *j["rule"])
            ctx.reads_edist_best_batch_async(ptr, j["d_off"], count, total, k, dq, nq, bq, be, bd)
            ctx.reads_edist_adapter_batch_async(ptr, j["d_off"], count, total, k, dq, nq, *j["full"].ptrs(), k, 1, 1)
            ctx.reads_edist_start_batch_async(ptr, j["d_off"], count, total, k, dq, nq, bq, be, st, sd)
        else:
            heads = [(ptr, n, count), (wptr, n, count)]
            fn = [ctx.reads_edist_adapter_async, ctx.reads_edist_adapter_packed_async, ctx.reads_pattern_edist_adapter_async,
                  ctx.reads_pattern_edist_adapter_packed_async][form]
            fn(*heads[form % 2], k, dp if form >= 2 else dq, nq, *j["out"].ptrs(), *j["rule"])
            ctx.reads_edist_best_async(ptr, n, count, k, dq, nq, bq, be, bd)
            ctx.reads_edist_adapter_async(ptr, n, count, k, dq, nq, *j["full"].ptrs(), k, 1, 1)
            ctx.reads_edist_start_async(ptr, n, count, k, dq, nq, bq, be, st, sd)
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, s, off, queries = j["i"], j["s"], j["off"], j["queries"]
        want = ao.reads_edist_adapter_batch(s, off, k, queries, *j["rule"])
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        full, best, start = j["full"].read(), j["best"].read(), j["start"].read()
        assert np.array_equal(full[0], best[0]) and np.array_equal(full[2], best[2]) and np.array_equal(full[4], best[4]), i
        assert np.array_equal(full[1], start[1]) and np.array_equal(full[4], start[4]), i
        assert (full[3][full[0] != ao.NO_U32] == k).all() and (full[3][full[0] == ao.NO_U32] == 255).all(), i


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """900,000 reads of 150 bases (135 * 10^6 bases: two chunks of the ASCII form, whose first holds 128 Mi / 150 reads; the packed form's chunks are cut
    at 4 Mi words / 5), k = 16, two adapters, on a context with the default dispatch; the reads on both sides of each boundary end with a planted overhang.
    The oracle runs on the reads around the boundaries, the first and the last ones; everywhere else the two-chunk results must equal the _async form's on
    the whole batch.  20,000 reads run in one chunk.  Then an N past the boundary reports its absolute index."""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    count, n, k = 900_000, 150, 16
    rule = (3, 1, 10)
    per_ascii, per_packed = (128 << 20) // n, ((128 << 20) // 32) // 5
    assert 0 < per_packed < per_ascii < count
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=count * n, dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    for per in (per_ascii, per_packed):
        codes[per * n - 9:per * n] = qc[0][:9]                          # the chunk's last read ends with nine positions of adapter 0
        codes[(per + 1) * n - 12:(per + 1) * n] = qc[1][:12]            # the next chunk's first read with twelve of adapter 1
    s = ro.LUT[codes]
    del codes
    rows = np.unique(np.concatenate([np.arange(200), np.arange(count - 200, count)] + [np.arange(per - 100, per + 100) for per in (per_ascii, per_packed)]))
    sample = np.ascontiguousarray(s.reshape(count, n)[rows]).reshape(-1)
    want = ao.reads_edist_adapter(sample, n, rows.size, k, queries, *rule)
    for per in (per_ascii, per_packed):
        at = int(np.searchsorted(rows, per))
        assert [tuple(int(a[r]) for a in want) for r in (at - 1, at)] == [(0, n - 9, n, 9, 0), (1, n - 12, n, 12, 0)]
    c = bn.Context(0)
    try:
        words = ro.pack_reads(s, n, count)
        t, ptr = _ascii_dev(s, 0)
        o = Out(count)
        torch.cuda.synchronize()
        c.reads_edist_adapter_async(ptr, n, count, k, _dev_queries(queries), 2, *o.ptrs(), *rule)
        dev = o.read(c)
        del t, o
        assert _same(tuple(a[rows] for a in dev), want)
        off = rb.offsets_of([n] * count)
        for got in (c.reads_edist_adapter(s, n, k, queries, *rule), c.reads_edist_adapter_packed(words, n, count, k, queries, *rule),
                    c.reads_pattern_edist_adapter_packed(words, n, count, k, rp.singletons(queries, k), *rule), c.reads_edist_adapter_batch(s, off, k, queries, *rule),
                    c.reads_edist_adapter_batch_packed(words, rb.word_offsets_of(off), off, k, queries, *rule)):
            assert _same(tuple(a[rows] for a in got), want), _diff(tuple(a[rows] for a in got), want)
            assert _same(got, dev)
        m = 20_000  # 6 * 10^6 base-query pairs: one chunk through the device
        assert _same(c.reads_edist_adapter(s[:m * n], n, k, queries, *rule), tuple(a[:m] for a in dev))
        assert _same(c.reads_pattern_edist_adapter_batch(s[:m * n], off[:m + 1], k, rp.singletons(queries, k), *rule), tuple(a[:m] for a in dev))
        assert _same(c.reads_pattern_edist_adapter(s[:m * n], n, k, rp.singletons(queries, k), *rule), tuple(a[:m] for a in dev))
        assert _same(c.reads_pattern_edist_adapter_batch_packed(words[:m * 5], rb.word_offsets_of(off[:m + 1]), off[:m + 1], k, rp.singletons(queries, k), *rule),
                     tuple(a[:m] for a in dev))
        bad_at = (per_ascii + 1) * n + 149
        s[bad_at] = ord("N")
        for call in (lambda: c.reads_edist_adapter(s, n, k, queries, *rule), lambda: c.reads_edist_adapter_batch(s, off, k, queries, *rule)):
            with pytest.raises(bn.NucleotideError) as ei:
                call()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
            del ei
    finally:
        c.close()


def test_cpp_mirror_of_the_adapter_forms(ctx, tmp_path):
    """the eight reads_*edist_adapter* methods of include/bitnuc.hpp against the definition, via tests/cpp/test_reads_edist_adapter_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_reads_edist_adapter_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_reads_edist_adapter_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ---- 3. identities ---------------------------------------------------------------------------------------------------------------------------

def test_identities_on_the_device(ctx):
    """1: min_overlap = k and rate 1/1 is the whole-read best match with its start (test_mixed_queue...); 2: rate 0/1 and min_overlap 1 is plain string
    matching; 3: singleton patterns equal the exact form; 4 and 6: _check_both everywhere above; 5: dist is the Levenshtein distance of the prefix to
    read[cut:end]"""
    rng = np.random.default_rng(55)
    k, n, count = 16, 120, 300
    queries, s, off = cases.random_reads(rng, [n] * count, k, 5)
    pats = rp.singletons(queries, k)
    codes = ro.codes_of(s).reshape(count, n)
    for rule in ((3, 1, 10), (1, 1, 5), (1, 0, 1)):
        a, p = _fixed(ctx, s, n, count, k, queries, rule, aoff=1, woff=1)
        pa, pp = _fixed(ctx, s, n, count, k, pats, rule, aoff=7, woff=0, pattern=True)
        ra, rp_ = _ragged(ctx, s, off, k, pats, rule, aoff=15, woff=1, pattern=True)
        assert _same(a, p) and _same(a, pa) and _same(a, pp) and _same(a, ra) and _same(a, rp_)
        adapter, cut, end, overlap, dist = a
        hit = np.nonzero(adapter != ao.NO_U32)[0]
        assert hit.size > count // 4
        for r in hit:
            assert ao.lev(ao.sets_of(pats[adapter[r]], int(overlap[r])), codes[r, cut[r]:end[r]]) == dist[r], r
        if rule == (1, 0, 1):
            text = bytes(s & 0xDF).decode()
            names = ["".join("ACGT"[c] for c in ro.query_codes(q, k)) for q in queries]
            for r in range(count):
                read = text[r * n:(r + 1) * n]
                found = None
                for q, name in enumerate(names):
                    at = read.find(name)
                    cand = (0, q, at + k, k) if at >= 0 else max(((k - i, q, n, i) for i in range(1, k) if read.endswith(name[:i])), key=lambda c: c[3], default=None)
                    if cand is not None and (found is None or cand < found):
                        found = cand
                if found is None:
                    assert adapter[r] == ao.NO_U32, r
                else:
                    assert (adapter[r], end[r], overlap[r], dist[r], cut[r]) == (found[1], found[2], found[3], 0, found[2] - found[3]), r


def test_seeded_differential_fuzz(ctx):
    rng = np.random.default_rng(20261)
    for it in range(24):
        k = int(rng.choice([1, 2, 3, 7, 16, 17, 31, 32]))
        nq = int(rng.integers(1, 12))
        rule = (int(rng.integers(1, k + 1)),) + RATES[int(rng.integers(0, 4))]
        count = int(rng.integers(1, 200))
        pattern = bool(it % 3 == 2)
        if it % 2:
            lengths = rng.integers(0, int(rng.choice([40, 150, 300])), size=count)
            queries, s, off = cases.random_reads(rng, lengths, k, nq)
            q = rp.singletons(queries, k) if pattern else queries
            if pattern:
                q = q.copy()
                q[0, :] |= np.uint32(1 << (k // 2))  # a position that takes any base
            _check_ragged(ctx, s, off, k, q, rule, aoff=OFFS[it % 4], woff=it % 2, tag=it, pattern=pattern)
        else:
            n = int(rng.integers(k, 200))
            queries, s, off = cases.random_reads(rng, [n] * count, k, nq)
            q = rp.singletons(queries, k) if pattern else queries
            _check_both(ctx, s, n, count, k, q, rule, tag=it, i=it, pattern=pattern)
