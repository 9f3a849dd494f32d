"""GPU tests of the indel-tolerant anchored match per read of a ragged batch (bitnuc_reads_edist_anchored_batch[_packed]_async, the pattern twins and the
host forms above the cutoff; reads_edist_kernel under its ragged layout policy, scan_edist_device.h) against tests/reads_edist_batch_oracle.py (the ragged
Hamming oracle's windows, the plain DP on each read's own span).  One read per lane; a lane loads its own table entries and its own span; the recurrence
loop runs wave-uniformly over the widest span among the wave's 64 lanes with Eq forced to 0 behind a shorter span; a wave whose lanes all have the widest
span the arguments allow takes the fixed form's loop.  So: counts around the wave and the block and one beyond the bounded grid; waves whose 64 lanes all
have different spans (0 included), waves of full spans only and waves without any window; k in {1, 2, 15, 16, 17, 31, 32} with widest spans in {k, k + 1,
31, 32, 33, 63, 64}; packed spans inside one word and across one and two boundaries with the first span base at every value mod 32; Q around the
interleave factor and the limit; the overhang traps (a copy of a query completed by the next read's first bases, the previous read's last bases, the pad
bits or the bytes behind the batch must not score 0); planted indels, ties, duplicates, all-N, empty-set and singleton patterns; fills; invalid bytes
inside and outside the spans; NULL second pointers; argument errors in their order; a hipGraph replay after the lengths, reads and queries changed; a
queue mixed with reads_hdist_anchored_batch_async and reads_edist_anchored_async; the host forms in one chunk and across two; the bitnuc.hpp methods; the
identities with the fixed form and the <= -Hamming inequality; a seeded differential fuzz whose inputs are required to hold indels, shortened spans and
reads without a window.  ASCII at byte offsets +0 / +1 / +7 / +15 with lowercase bases and packed words at 16-byte and 8-mod-16 offsets with junk pad bits
run on the same data.  Every comparison is exact equality of all written arrays; guard words and bytes surround all six outputs and both dist arrays start
at odd byte offsets."""
import numpy as np
import pytest

import pattern_oracle as po
import reads_anchored_batch_oracle as rab
import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_batch_oracle as ebo
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

pytestmark = pytest.mark.gpu

GUARD = 8
FILL32 = 0x5A5A5A5A
DOFFS = (3, 5)
OFFS = (0, 1, 7, 15)
START, END = 0, 1
BOTH = (START, END)
U = 4  # kEdistInterleave (bitnuc_amd/csrc/edist_step_device.h)


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _dev_queries(queries, pattern=False):
    import torch
    if pattern:
        return torch.from_numpy(rp.as_patterns(queries).view(np.int32).copy()).to("cuda:0")
    return _dev_u64(np.asarray(queries, dtype=np.uint64).reshape(-1))


class Out:
    """`triples` x (query / end with GUARD words before and after [0, count); dist inside a guarded buffer, starting at an odd byte)"""

    def __init__(self, count, triples=2):
        import torch
        self.count = count
        self.w = [torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(2 * triples)]
        self.d = [torch.full((off + count + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0") for off in DOFFS[:triples]]

    def ptrs(self, triples=None):
        out = []
        for j, d in enumerate(self.d[:triples]):
            out += [self.w[2 * j].data_ptr() + 4 * GUARD, self.w[2 * j + 1].data_ptr() + 4 * GUARD, d.data_ptr() + DOFFS[j]]
        return out

    def reset(self):
        for a in self.w:
            a.fill_(FILL32)
        for a in self.d:
            a.fill_(0x5A)

    def untouched(self, triples=(0, 1)):
        return all(bool((self.w[2 * j + i] == FILL32).all()) for j in triples for i in (0, 1)) and all(bool((self.d[j] == 0x5A).all()) for j in triples)

    def read(self, ctx=None):
        if ctx is not None:
            ctx.sync()
        n = self.count
        out = []
        for j, d in enumerate(self.d):
            for a in self.w[2 * j:2 * j + 2]:
                a = a.cpu().numpy().view(np.uint32)
                assert (a[:GUARD] == FILL32).all() and (a[GUARD + n:] == FILL32).all(), "query / end written outside [0, count)"
                out.append(a[GUARD:GUARD + n].copy())
            d = d.cpu().numpy()
            assert (d[:DOFFS[j]] == 0x5A).all() and (d[DOFFS[j] + n:] == 0x5A).all(), "dist written outside [0, count)"
            out.append(d[DOFFS[j]:DOFFS[j] + n].copy())
        return tuple(out)


def _ascii_dev(s, off, behind=None):
    """s at byte offset `off` of a device buffer; `behind`: the bytes right behind the batch (default zeros: invalid, must never be examined)"""
    import torch
    t = torch.zeros(s.size + off + 16, dtype=torch.uint8, device="cuda:0")
    if s.size:
        t[off:off + s.size] = torch.from_numpy(s)
    if behind is not None:
        t[off + s.size:off + s.size + len(behind)] = torch.from_numpy(np.asarray(behind, dtype=np.uint8))
    return t, t.data_ptr() + off


def _words_dev(w, off):
    import torch
    t = torch.zeros(w.size + off + 2, dtype=torch.int64, device="cuda:0")
    if w.size:
        t[off:off + w.size] = torch.from_numpy(w.view(np.int64))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    bad = np.nonzero(np.any([g != w for g, w in zip(got, want)], axis=0))[0]
    return [(int(r), tuple(int(a[r]) for a in got), tuple(int(a[r]) for a in want)) for r in bad[:5]]


def _row(want, r):
    return tuple(int(a[r]) for a in want)


def _fns(ctx, pattern):
    return (ctx.reads_pattern_edist_anchored_batch_async, ctx.reads_pattern_edist_anchored_batch_packed_async) if pattern else \
           (ctx.reads_edist_anchored_batch_async, ctx.reads_edist_anchored_batch_packed_async)


def _both(ctx, s, off, k, queries, anchor, lo, hi, aoff=0, woff=0, words=None, behind=None, pattern=False):
    """(six arrays of the ASCII form, six of the packed form), guards checked"""
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint64)
    count, nq = off.size - 1, len(queries)
    wtab = rb.word_offsets_of(off)
    w = rb.pack_batch(s, off, seed=k) if words is None else words
    t, ptr = _ascii_dev(s, aoff, behind)
    tw, wptr = _words_dev(w, woff)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_queries(queries, pattern)
    o1, o2 = Out(count), Out(count)
    fa, fp = _fns(ctx, pattern)
    torch.cuda.synchronize()
    fa(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
    fp(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
    ctx.sync()
    got = o1.read(), o2.read()
    del t, tw
    return got


def _check(ctx, s, off, k, queries, anchor, lo, hi, want=None, aoff=0, woff=0, words=None, behind=None, tag=(), pattern=False):
    if want is None:
        want = (ebo.reads_pattern_edist_batch if pattern else ebo.reads_edist_batch)(s, off, k, queries, anchor, lo, hi)
    a, p = _both(ctx, s, off, k, queries, anchor, lo, hi, aoff, woff, words, behind, pattern)
    assert _same(a, want), ("ascii", tag, _diff(a, want))
    assert _same(p, want), ("packed", tag, _diff(p, want))
    return want


def _ascii(codes):
    return ro.LUT[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


def _wave_lengths(rng, count, k, lo, width):
    """lengths in waves of 64 consecutive reads that have as many different numbers of admissible offsets as the range allows (n = min(len - k - lo,
    width - 1) + 1 for either anchor: 0 at k + lo - 1 bases, width from k + lo + width - 1 on; all 64 different when width >= 63), with empty reads,
    reads of k - 1 and k bases and much longer ones filling the rest"""
    base = k + lo - 1
    out = []
    while len(out) < count:
        wave = [base + j for j in range(min(64, width + 1))]
        while len(wave) < 64:
            wave.append(int(rng.choice((0, max(k - 1, 0), k, base + width, base + width + 1, base + width + int(rng.integers(2, 200))))))
        rng.shuffle(wave)
        out += wave
    return out[:count]


def _plant(rng, s, off, k, queries, anchor, lo, hi, share=0.8):
    """a copy of a query with 1 .. 3 edits, at least one of them an indel, inside the span of about `share` of the reads whose span has >= k + 1 bases"""
    first, n = rab.windows(np.diff(np.asarray(off).astype(np.int64)), k, anchor, lo, hi)
    o = np.asarray(off).astype(np.int64)
    rows = np.nonzero(n >= 2)[0]
    if rows.size > 400:
        rows = rng.choice(rows, size=400, replace=False)
    for r in rows:
        if rng.random() >= share:
            continue
        span = int(n[r]) + k - 1
        c = eo.plant(rng, ro.query_codes(queries[int(rng.integers(0, len(queries)))], k), int(rng.integers(1, 4)))[:span]
        at = int(o[r]) + int(first[r]) + int(rng.integers(0, span - len(c) + 1))
        s[at:at + len(c)] = _ascii(c)


def _random(rng, lengths, k, nq, anchor=None, lo=0, hi=0):
    queries = ro.random_queries(rng, nq, k)
    s, off = rb.random_batch(rng, lengths, k, queries)
    if anchor is not None:
        _plant(rng, s, off, k, queries, anchor, lo, hi)
    return queries, s, off


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 63, 64, 65, 255, 257))
def test_counts_around_the_wave_and_the_block(ctx, count):
    rng = np.random.default_rng(100 + count)
    for i, (k, nq, lo, width) in enumerate(((16, 9, 0, 4), (31, 3, 2, 11), (5, 33, 0, 1))):
        lengths = _wave_lengths(rng, count, k, lo, width)
        for anchor in BOTH:
            queries, s, off = _random(rng, lengths, k, nq, anchor, lo, lo + width - 1)
            _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[(i + count) % 4], woff=(i + count) % 2, tag=(count, k, lo, width, anchor))


def test_a_count_beyond_the_bounded_grid(ctx):
    """more reads than the grid has lanes (at most 8 workgroups of 256 lanes per CU): some lanes walk two reads, with the second read's table entries
    loaded one trip ahead; reads of 0 .. 24 bases"""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 4161
    rng = np.random.default_rng(5)
    k, nq = 6, 3
    queries, s, off = _random(rng, rng.integers(0, 25, size=count), k, nq, END, 0, 3)
    _check(ctx, s, off, k, queries, END, 0, 3, aoff=1, woff=1)
    _check(ctx, s, off, k, queries, START, 9, 12, aoff=7, woff=0)


@pytest.mark.parametrize("k,width", ((1, 64), (2, 63), (8, 57), (32, 33)))
def test_the_64_lanes_of_a_wave_all_have_different_spans(ctx, k, width):
    """k = 1 / 2 with 64 / 63 offsets: the 64 reads of a wave have the numbers of admissible offsets 0 .. 63 in a random order (rab.lengths_all_n and
    waves of 64 consecutive lengths); narrower ranges: as many as there are.  Three waves and a partial one; a wave of full spans only (the fixed loop)
    and a wave without any window follow."""
    rng = np.random.default_rng(900 + k)
    for lo in (0, 3):
        lengths = _wave_lengths(rng, 64 * 3 + 17, k, lo, width)
        lengths += [k + lo + width - 1 + int(x) for x in rng.integers(0, 50, size=64)] + [int(x) for x in rng.integers(0, k + lo, size=64)]
        lengths += rab.lengths_all_n(k, lo, width)
        for anchor in BOTH:
            queries, s, off = _random(rng, lengths, k, 5, anchor, lo, lo + width - 1)
            n = rab.windows(lengths, k, anchor, lo, lo + width - 1)[1]
            if width >= 63:
                assert all(len(set(n[64 * w:64 * w + 64].tolist())) == 64 for w in range(3))
            assert (n[64 * 3 + 17:64 * 4 + 17] == width).all() and (n[64 * 4 + 17:64 * 5 + 17] == 0).all()
            _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[(k + lo) % 4], woff=lo & 1, tag=(k, width, lo, anchor))


@pytest.mark.parametrize("k", (1, 2, 15, 16, 17, 31, 32))
def test_k_and_spans_around_the_registers(ctx, k):
    """widest spans in {k, k + 1, 31, 32, 33, 63, 64}; the reads' own spans n_r + k - 1 end inside, at the end of and just behind a register of 16 bases"""
    rng = np.random.default_rng(300 + k)
    for i, span in enumerate(sorted({k, k + 1, 31, 32, 33, 63, 64})):
        if span < k:
            continue
        width = span - k + 1
        lo = (0, 1, 2, 3)[(i + k) % 4]
        nq = (1, 2, 3, 5, 7, 8, 9)[i % 7]
        need = k + lo
        lengths = [need + j for j in (0, 15 - k, 16 - k, 17 - k, 31 - k, 32 - k, 33 - k, 47 - k, 48 - k, 49 - k, 63 - k, 64 - k) if j >= 0]  # spans of 16, 17, ...
        lengths += _wave_lengths(rng, 70 - len(lengths), k, lo, width)
        rng.shuffle(lengths)
        anchor = BOTH[(i + k) % 2]
        queries, s, off = _random(rng, lengths, k, nq, anchor, lo, lo + width - 1)
        _check(ctx, s, off, k, queries, anchor, lo, lo + width - 1, aoff=OFFS[i % 4], woff=i % 2, tag=(k, span, lo, nq, anchor))
        _check(ctx, s, off, k, queries, 1 - anchor, lo, lo + width - 1, aoff=OFFS[(i + 1) % 4], woff=(i + 1) % 2, tag=(k, span, lo, nq, 1 - anchor))


@pytest.mark.parametrize("nq", (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 33))
def test_queries_around_the_interleave_factor(ctx, nq):
    rng = np.random.default_rng(400 + nq)
    k, lo, width = 16, 0, 8
    lengths = _wave_lengths(rng, 130, k, lo, width)
    queries, s, off = _random(rng, lengths, k, nq, END, lo, lo + width - 1)
    if nq >= 2:
        queries[nq - 1] = queries[0] ^ (np.uint64(1) << np.uint64(63))  # the last query of the last group: an equal duplicate of query 0
    _check(ctx, s, off, k, queries, END, lo, lo + width - 1, aoff=OFFS[nq % 4], woff=nq % 2, tag=nq)
    _check(ctx, s, off, k, rp.singletons(queries, k), END, lo, lo + width - 1, aoff=OFFS[nq % 4], woff=nq % 2, tag=nq, pattern=True)


def test_packed_spans_in_one_word_and_across_boundaries_with_every_first_base_mod_32(ctx):
    """END anchor: a_r = len_r - k - pos_hi follows the read's length, so 64 consecutive lengths put the span's first base at every value mod 32, twice;
    spans of 10, 33 and 64 bases lie inside one word or cross one and two boundaries"""
    rng = np.random.default_rng(23)
    k = 9
    for width, lo in ((2, 0), (25, 0), (56, 0), (56, 3), (12, 31)):
        base = k + lo + width - 1
        lengths = [base + j for j in range(64)] + [max(0, base - 1 - j) for j in range(0, 30, 3)]
        rng.shuffle(lengths)
        queries, s, off = _random(rng, lengths, k, 6, END, lo, lo + width - 1)
        first = rab.windows(lengths, k, END, lo, lo + width - 1)[0]
        assert set((first % 32).tolist()) == set(range(32))
        for woff in (0, 1):
            _check(ctx, s, off, k, queries, END, lo, lo + width - 1, woff=woff, aoff=OFFS[width % 4], tag=(width, lo))
        _check(ctx, s, off, k, queries, START, lo, lo + width - 1, woff=1, tag=(width, lo, "start"))


def test_fills_empty_reads_no_window_and_count_zero(ctx):
    import torch
    rng = np.random.default_rng(31)
    k = 8
    lengths = [0, 0, 40, 7, 0, 12, 8, 0, 90, 3, 0, 0]  # empty reads at the start, in the middle and at the end
    queries, s, off = _random(rng, lengths, k, 3)
    count = len(lengths)
    for anchor in BOTH:
        want = _check(ctx, s, off, k, queries, anchor, 0, 3, aoff=1, woff=1)
        assert list(want[2] == 0xFF) == [True, True, False, True, True, False, False, True, False, True, True, True]
        short = rb.offsets_of([0, 3, 7, 5, 0, 1] * 20)  # a batch in which no read has a window, but the batch has k + pos_lo bases
        ss = s[:int(short[-1])] if s.size >= int(short[-1]) else np.resize(s, int(short[-1]))
        assert _same(_check(ctx, ss, short, k, queries, anchor, 0, 3, aoff=7), eo.fill6(120))
        for kk, qq, lo, hi in ((0, queries, 0, 3), (k, queries[:0], 0, 3), (k, queries, 5, 4), (k, queries, 100, 103), (k, queries, 2**40, 2**40 + 3)):
            want = ebo.reads_edist_batch(s, off, kk, qq, anchor, lo, hi)
            assert _same(want, eo.fill6(count))
            _check(ctx, s, off, kk, qq, anchor, lo, hi, want, aoff=1, woff=1, tag=(kk, lo, hi))
    o = Out(count)  # count == 0: nothing written
    t, ptr = _ascii_dev(s, 0)
    torch.cuda.synchronize()
    ctx.reads_edist_anchored_batch_async(ptr, _dev_u64(off), 0, int(off[-1]), k, _dev_queries(queries), 3, *o.ptrs(), pos_lo=0, pos_hi=3)
    ctx.sync()
    assert o.untouched()


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 31, 32))
def test_the_overhang_traps(ctx, k):
    """START 0 .. 4 (the full span: k + 4 bases).  Read 0 is two bases short of k + 4 and ends in the query's first k - 2 bases; what follows -- the next
    read's first bases, the pad bits of its last word, the bytes behind the batch when it is the last read -- completes a perfect copy.  The END mirror:
    a read shorter than k + pos_hi begins with the query's last k - 2 bases, the previous read ends in its first two.  Neither may score 0.  And a copy
    with one base deleted exactly fills a span of k - 1 + 1 bases."""
    rng = np.random.default_rng(k)
    g = 2
    q = rng.integers(0, 4, size=k)
    q[:3], q[-3:] = (0, 1, 3), (3, 1, 0)  # no G at either end: the background cannot stand in for a missing base
    queries = np.array([ro.word_of(q)], dtype=np.uint64)
    r0 = np.r_[[g] * 4, q[:k - 2]]               # k + 2 bases, the copy's first k - 2 at its end
    r1 = np.r_[q[k - 2:], [g] * (k + 10)]        # begins with the copy's last two
    r2 = np.r_[[g] * (k + 10), q[:2]]            # ends in the copy's first two
    r3 = np.r_[q[2:], [g] * 4]                   # k + 2 bases, begins with the copy's last k - 2
    r4 = np.delete(q, 3)                         # k - 1 bases: no window at all, although the next read would complete it
    r5 = np.r_[q[k - 1:], [g] * (k + 3)]
    reads = [r0, r1, r2, r3, r4, r5, r0]         # and read 0 once more as the LAST read: the bytes behind the batch complete it
    s = _ascii(np.concatenate(reads))
    off = rb.offsets_of([len(r) for r in reads])
    pads = {0: list(q[k - 2:]), 2: list(q[2:]), 3: list(q[k - 2:]), 4: list(q[k - 1:]), 6: list(q[k - 2:])}
    words = rb.pack_batch(s, off, pad_codes=pads, seed=3)
    behind = _ascii(np.r_[q[k - 2:], [g] * 6])
    for anchor in BOTH:
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, 0, 4)
        assert int(want[2][0]) == 2 and int(want[2][3]) == 2 and int(want[2][4]) == 0xFF and int(want[2][6]) == 2, want  # two edits, never 0
        for aoff in OFFS:
            _check(ctx, s, off, k, queries, anchor, 0, 4, want, aoff=aoff, woff=aoff & 1, words=words, behind=behind, tag=(k, anchor, aoff))
    reads = [np.r_[[g], np.delete(q, 3)], np.r_[[g] * 40]]  # one base deleted: k - 1 bases exactly filling the span of a read of k bases behind its first
    s = _ascii(np.concatenate(reads))
    off = rb.offsets_of([len(r) for r in reads])
    for anchor in BOTH:
        want = _check(ctx, s, off, k, queries, anchor, 0, 3, aoff=1)
        assert (int(want[2][0]), int(want[1][0])) == (1, k)


def test_planted_indels_in_reads_of_different_lengths(ctx):
    k, read_len, lo, n, s, queries = eo.planted_cases()
    cut = (40, 45, 52, 60, 33)  # each keeps the copy whole; the last read has a shortened span
    b = np.concatenate([s[r * read_len:r * read_len + c] for r, c in enumerate(cut)])
    off = rb.offsets_of(cut)
    want = _check(ctx, b, off, k, queries, START, lo, lo + n - k, aoff=7, woff=1)
    assert [list(want[i]) for i in range(3)] == [[1] * 5, [29, 31, 30, 30, 30], [1, 1, 1, 2, 0]]
    _check(ctx, b, off, k, rp.singletons(queries, k), START, lo, lo + n - k, want, aoff=1, pattern=True)
    ham = rab.reads_anchored_batch(b, off, k, queries, START, lo, lo + n - k)
    assert (want[2] <= ham[2]).all() and (want[2][:2] < ham[2][:2]).all()
    want = _check(ctx, b, off, k, queries, END, 0, 14, aoff=15)
    assert list(want[1][[0, 4]]) == [29, 30] and list(want[2][[0, 4]]) == [1, 0]


def test_ties_two_ends_two_queries_and_a_duplicate(ctx):
    k = 6
    q = np.array([0, 1, 2, 3, 1, 0])
    codes = np.full(40, 2)
    codes[5:11], codes[20:26] = q, q
    s = np.concatenate([_ascii(codes), _ascii(codes[:30]), _ascii(codes[8:])])  # 40, 30 and 32 bases
    off = rb.offsets_of([40, 30, 32])
    far = ro.word_of([3] * k)
    queries = np.array([far, ro.word_of(q), far, ro.word_of(q) | (1 << 40), far], dtype=np.uint64)
    want = _check(ctx, s, off, k, queries, START, 0, 58 - k, aoff=15)
    assert [_row(want, r) for r in range(3)] == [(1, 11, 0, 3, 11, 0), (1, 11, 0, 3, 11, 0), (1, 18, 0, 3, 18, 0)]  # the smaller end; the equal duplicate
    want = _check(ctx, s, off, k, queries, END, 0, 14, woff=1)  # the last 20 bases of each read
    assert _row(want, 0) == (1, 26, 0, 3, 26, 0) and int(want[1][2]) == 18
    near = q.copy()
    near[2] = 0
    queries = np.array([ro.word_of(near), far, ro.word_of(near)], dtype=np.uint64)
    want = _check(ctx, s, off, k, queries, START, 0, 30, woff=1)
    assert _row(want, 0) == (0, 11, 1, 2, 11, 1)  # two queries at the same distance: the smaller index
    want = _check(ctx, s, off, k, queries[:1], START, 0, 30)
    assert _row(want, 0) == (0, 11, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF)  # one query: the fill in the second triple


@pytest.mark.parametrize("k,lo,hi", ((1, 3, 9), (12, 7, 30), (32, 0, 32)))
def test_patterns_all_n_empty_set_and_singletons(ctx, k, lo, hi):
    rng = np.random.default_rng(0x9A7 + k)
    lengths = _wave_lengths(rng, 77, k, lo, hi - lo + 1)
    queries, s, off = _random(rng, lengths, k, 5)
    for anchor in BOTH:
        first, n = rab.windows(lengths, k, anchor, lo, hi)
        has = n > 0
        exact = _check(ctx, s, off, k, queries, anchor, lo, hi, aoff=1)
        sing = rp.singletons(queries, k)
        _check(ctx, s, off, k, sing, anchor, lo, hi, exact, aoff=7, woff=1, pattern=True)  # byte for byte the exact form
        all_n = po.from_iupac("N" * k)
        want = _check(ctx, s, off, k, [all_n, sing[0]], anchor, lo, hi, pattern=True)
        assert (want[0][has] == 0).all() and (want[1][has] == (first + k)[has]).all() and (want[2][has] == 0).all()
        sets = [po.random_sets(rng, k) for _ in range(6)]
        sets[2] = [set() if i == k // 2 else x for i, x in enumerate(sets[2])]
        sets[5] = [set()] * k  # matches nothing: distance k at the first end
        pats = rp.as_patterns([po.from_sets(x) for x in sets])
        _check(ctx, s, off, k, pats, anchor, lo, hi, aoff=15, pattern=True)
        want = _check(ctx, s, off, k, pats[5:], anchor, lo, hi, pattern=True)
        assert (want[2][has] == k).all() and (want[1][has] == (first + 1)[has]).all() and (want[2][~has] == 0xFF).all()


# ---- 3. the contract --------------------------------------------------------------------------------------------------------------------------
def test_null_second_pointers_write_the_best_triple_only(ctx):
    import torch
    rng = np.random.default_rng(9)
    k, nq = 13, 10
    queries, s, off = _random(rng, _wave_lengths(rng, 99, k, 0, 6), k, nq, END, 0, 5)
    count = off.size - 1
    wtab = rb.word_offsets_of(off)
    want = ebo.reads_edist_batch(s, off, k, queries, END, 0, 5)
    t, ptr = _ascii_dev(s, 1)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 1)
    d_off, d_wtab, dq = _dev_u64(off), _dev_u64(wtab), _dev_queries(queries)
    for packed in (False, True):
        o = Out(count)
        torch.cuda.synchronize()
        if packed:
            ctx.reads_edist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o.ptrs(1), pos_lo=0, pos_hi=5, anchor="end")
        else:
            ctx.reads_edist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(1), pos_lo=0, pos_hi=5, anchor="end")
        ctx.sync()
        assert o.untouched(triples=(1,)) and _same(o.read()[:3], want[:3])


def _raw_err(ctx, packed, head, k, anchor, lo, hi, dq, nq, six, pattern=False):
    """(status, value) of a device call through the raw entry point (the Python error carries no value for Unsupported)"""
    import ctypes as C
    from bitnuc_amd import _lib as L
    raw = getattr(L.load(), "bitnuc_reads_" + ("pattern_" if pattern else "") + "edist_anchored_batch" + ("_packed" if packed else "") + "_async")
    err = L.BitnucErr()
    st = raw(ctx._h, *(C.c_void_p(p) if i < (3 if packed else 2) else p for i, p in enumerate(head)), k, anchor, lo, hi, C.c_void_p(dq.data_ptr()), nq,
             *(C.c_void_p(p) if p else None for p in six), C.byref(err))
    return st, int(err.value)


def test_argument_errors_in_their_order_leave_the_outputs_untouched(ctx):
    import torch
    from bitnuc_amd import _lib as L
    rng = np.random.default_rng(2)
    k = 12
    queries, s, off = _random(rng, rng.integers(0, 150, size=100), k, 16)
    count, total = 100, int(off[-1])
    wtab = rb.word_offsets_of(off)
    t, ptr = _ascii_dev(s, 0)
    tw, wptr = _words_dev(rb.pack_batch(s, off), 0)
    d_off, d_wtab = _dev_u64(off), _dev_u64(wtab)
    o = Out(count)
    six = o.ptrs()
    size_max = 2**64 - 1
    torch.cuda.synchronize()
    for pattern in (False, True):
        dq = _dev_queries(rp.singletons(queries, k) if pattern else queries, pattern)
        for packed, head in ((False, (ptr, d_off.data_ptr(), count, total)), (True, (wptr, d_wtab.data_ptr(), d_off.data_ptr(), count, int(wtab[-1])))):
            def err(head, k_, anchor, lo, hi, nq, six_):
                return _raw_err(ctx, packed, head, k_, anchor, lo, hi, dq, nq, six_, pattern)
            assert err(head, 33, 7, 0, size_max, 65537, six) == (L.SEQUENCE_TOO_LONG, 33)  # k first
            big = head[:-1] + (2**58 if not packed else 2**53,)
            assert err(big, k, 7, 0, size_max, 65537, six) == (L.UNSUPPORTED, big[-1])     # then the totals' limit
            assert err(head, k, 7, 0, size_max, 65537, six) == (L.UNSUPPORTED, 65537)      # the query count
            assert err(head, k, 2, 0, size_max, 16, six) == (L.UNSUPPORTED, 2)             # the anchor
            assert err(head, k, END, 0, size_max, 16, six) == (L.UNSUPPORTED, size_max)    # the span
            assert err(head, k, END, 0, 53, 16, six) == (L.UNSUPPORTED, 65)
            for bad in ((six[0], six[1], six[2], 0, six[4], six[5]), (six[0], six[1], six[2], six[3], 0, 0), (six[0], six[1], six[2], six[3] + 2, six[4], six[5]),
                        (six[0], 0, six[2], six[3], six[4], six[5])):
                assert err(head, k, END, 0, 3, 16, bad) == (L.UNSUPPORTED, 0)
            for i in ((1,) if not packed else (1, 2)):  # a table NULL or not 8-byte aligned
                for v in (0, head[i] + 4):
                    assert err(head[:i] + (v,) + head[i + 1:], k, END, 0, 3, 16, six) == (L.UNSUPPORTED, 0)
            assert err((0,) + head[1:], k, END, 0, 3, 16, six) == (L.UNSUPPORTED, 0)      # the data, last
            if packed:
                assert err((wptr + 4,) + head[1:], k, END, 0, 3, 16, six) == (L.UNSUPPORTED, 0)
    ctx.sync()
    assert o.untouched()
    dq = _dev_queries(queries)
    room = 32 * int(wtab[-1])  # no window from the host-known arguments: the fill, even with NULL data
    for kk, nq, lo, hi in ((0, 16, 0, 3), (k, 0, 0, 3), (k, 16, 5, 4), (k, 16, room, room + 3)):
        for packed, head in ((False, (0, d_off.data_ptr(), count, total)), (True, (0, d_wtab.data_ptr(), d_off.data_ptr(), count, int(wtab[-1])))):
            o = Out(count)
            torch.cuda.synchronize()
            assert _raw_err(ctx, packed, head, kk, START, lo, hi, dq, nq, o.ptrs()) == (L.OK, 0)
            assert _same(o.read(ctx), eo.fill6(count)), (kk, nq, lo, hi)


def test_invalid_bytes_inside_and_outside_the_spans(ctx):
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(7)
    k, nq, lo, hi = 17, 9, 2, 5
    lengths = _wave_lengths(rng, 400, k, lo, 4)
    queries, s, off = _random(rng, lengths, k, nq)
    count = off.size - 1
    dq, d_off = _dev_queries(queries), _dev_u64(off)
    for anchor in BOTH:
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, lo, hi)
        mask = rab.span_bytes(off, k, anchor, lo, hi)
        b = s.copy()
        b[~mask] = rng.choice(np.frombuffer(b"Nn\x00\xffx-", dtype=np.uint8), size=int((~mask).sum()))  # every byte that no span holds is invalid: the byte
        # directly behind a short read's span and every byte of a read without a window among them
        for aoff in (0, 3):
            t, ptr = _ascii_dev(b, aoff)
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_edist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert _same(o.read(ctx), want)  # no error, correct results
        spans = np.nonzero(mask)[0]
        first_read = spans[spans < int(off[np.nonzero(np.diff(off.astype(np.int64)) >= k + lo)[0][0] + 1])]
        for bad_at, aoff in ((int(first_read[-1]), 0), (int(spans[0]), 9), (int(spans[-1]), 5), (int(spans[spans.size // 2]), 1)):
            c = b.copy()
            c[bad_at] = ord("N")
            later = spans[spans > bad_at + 300]
            if later.size:
                c[int(later[0])] = ord("x")  # a later one: the first in buffer order wins
            t, ptr = _ascii_dev(c, aoff)
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_edist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            with pytest.raises(bn.NucleotideError) as ei:
                ctx.sync()
            assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
            del ei
            ctx.sync()  # latched once: nothing is left for the next sync
            t2, ptr2 = _ascii_dev(b, aoff)  # the next call on the same context is clean and correct
            o = Out(count)
            torch.cuda.synchronize()
            ctx.reads_edist_anchored_batch_async(ptr2, d_off, count, int(off[-1]), k, dq, nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            assert _same(o.read(ctx), want)


def test_the_query_limit(ctx):
    """BITNUC_MAX_QUERIES queries on one read are accepted (the winner planted at the last index, its duplicate in the middle), one more is refused"""
    rng = np.random.default_rng(65537)
    k, nq = 20, 65536  # (k = 20: no random query comes within one edit of the read)
    queries = ro.random_queries(rng, nq, k)
    queries[30000] = queries[nq - 1] ^ (np.uint64(1) << np.uint64(60))
    codes = rng.integers(0, 4, size=28)
    codes[5:5 + k - 1] = np.delete(ro.query_codes(queries[nq - 1], k), 4)  # the last query with one base deleted
    s = _ascii(codes)
    off = rb.offsets_of([28])
    want = _check(ctx, s, off, k, queries, END, 0, 6, aoff=1, woff=1)  # the span: bases 2 .. 27
    assert _row(want, 0) == (30000, 5 + k - 1, 1, nq - 1, 5 + k - 1, 1)
    from bitnuc_amd import _lib as L
    o = Out(1)
    t, ptr = _ascii_dev(s, 0)
    d_off = _dev_u64(off)
    dq = _dev_queries(np.zeros(nq + 1, dtype=np.uint64))
    assert _raw_err(ctx, False, (ptr, d_off.data_ptr(), 1, 28), k, END, 0, 6, dq, nq + 1, o.ptrs()) == (L.UNSUPPORTED, nq + 1)
    ctx.sync()
    assert o.untouched()


def test_graph_replay_after_the_lengths_the_reads_and_the_queries_changed():
    """the tables are read on the device at every replay: the same count and totals, other lengths, reads and queries give the new answers"""
    import torch
    import bitnuc_amd as bn
    rng = np.random.default_rng(78)
    k, nq, lo, hi, count = 31, 9, 0, 3, 2000
    l1 = np.array(_wave_lengths(rng, count, k, lo, 4))
    l1[l1 % 32 == 0] += 1  # no multiple of 32: a permutation then keeps the words' total as well
    l2 = rng.permutation(l1)
    (q1, s1, off1), (q2, s2, off2) = _random(rng, l1, k, nq, END, lo, hi), _random(rng, l2, k, nq, END, lo, hi)
    w1tab, w2tab = rb.word_offsets_of(off1), rb.word_offsets_of(off2)
    assert int(off1[-1]) == int(off2[-1]) and int(w1tab[-1]) == int(w2tab[-1]) and not np.array_equal(off1, off2)
    want1, want2 = ebo.reads_edist_batch(s1, off1, k, q1, END, lo, hi), ebo.reads_edist_batch(s2, off2, k, q2, END, lo, hi)
    assert not np.array_equal(want1[1], want2[1])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = bn.Context(0, stream=st.cuda_stream)
        t, ptr = _ascii_dev(s1, 7)
        w = rb.pack_batch(s1, off1)
        tw, wptr = _words_dev(w, 1)
        dq, d_off, d_wtab = _dev_queries(q1), _dev_u64(off1), _dev_u64(w1tab)
        o1, o2 = Out(count), Out(count)

        def run():
            c.reads_edist_anchored_batch_async(ptr, d_off, count, int(off1[-1]), k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi, anchor="end")
            c.reads_edist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(w1tab[-1]), k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi, anchor="end")
        run()  # warm-up outside the capture: sizes the scratch
        assert _same(o1.read(c), want1) and _same(o2.read(c), want1)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                run()
            t[7:7 + s2.size] = torch.from_numpy(s2).to(t.device)
            tw[1:1 + w.size] = torch.from_numpy(rb.pack_batch(s2, off2).view(np.int64)).to(tw.device)
            dq.copy_(_dev_queries(q2))
            d_off.copy_(_dev_u64(off2))
            d_wtab.copy_(_dev_u64(w2tab))
            for _ in range(2):
                o1.reset()
                o2.reset()
                g.replay()
                assert _same(o1.read(c), want2) and _same(o2.read(c), want2)
        finally:
            g.reset()
            del g
            c.close()


def test_mixed_queue_with_one_sync(ctx):
    """the ragged edit-distance calls (ASCII, packed and pattern forms in turn, both anchors) between reads_hdist_anchored_batch_async and
    reads_edist_anchored_async calls on one context, different (count, n_queries) between consecutive calls (all three lay out scratch 10 anew), one sync
    at the end, every result checked afterwards"""
    import torch
    rng = np.random.default_rng(809)
    k = 21
    jobs = []
    for i, (count, nq) in enumerate(((500, 5), (40, 33), (2000, 1), (333, 17), (90, 40), (1200, 16), (7, 2), (800, 3))):  # inputs and outputs first
        lo, hi = ((0, 3), (2, 2), (1, 20))[i % 3]
        anchor = ("end", "start")[(i >> 1) & 1]
        lengths = rng.integers(0, 90, size=count) if i % 3 else np.full(count, 64)
        queries, s, off = _random(rng, lengths, k, nq, anchor, lo, hi)
        wtab = rb.word_offsets_of(off)
        jobs.append(dict(i=i, count=count, nq=nq, queries=queries, s=s, off=off, wtab=wtab, ascii=_ascii_dev(s, (0, 7, 1)[i % 3]), dq=_dev_queries(queries),
                         dp=_dev_queries(rp.singletons(queries, k), True), d_off=_dev_u64(off), d_wtab=_dev_u64(wtab), out=Out(count), ham=Out(count), fixed=Out(count),
                         wdev=_words_dev(rb.pack_batch(s, off), i & 1), anchor=anchor, rng=(lo, hi)))
    torch.cuda.synchronize()
    for j in jobs:  # the queue: nothing waits between these calls
        i, count, nq, ptr, dq, (lo, hi), an = j["i"], j["count"], j["nq"], j["ascii"][1], j["dq"], j["rng"], j["anchor"]
        total, wtotal = int(j["off"][-1]), int(j["wtab"][-1])
        if i % 4 == 0:
            ctx.reads_edist_anchored_batch_async(ptr, j["d_off"], count, total, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi, anchor=an)
        elif i % 4 == 1:
            ctx.reads_edist_anchored_batch_packed_async(j["wdev"][1], j["d_wtab"], j["d_off"], count, wtotal, k, dq, nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi, anchor=an)
        elif i % 4 == 2:
            ctx.reads_pattern_edist_anchored_batch_async(ptr, j["d_off"], count, total, k, j["dp"], nq, *j["out"].ptrs(), pos_lo=lo, pos_hi=hi, anchor=an)
        else:
            ctx.reads_pattern_edist_anchored_batch_packed_async(j["wdev"][1], j["d_wtab"], j["d_off"], count, wtotal, k, j["dp"], nq, *j["out"].ptrs(), pos_lo=lo,
                                                                pos_hi=hi, anchor=an)
        ctx.reads_hdist_anchored_batch_async(ptr, j["d_off"], count, total, k, dq, nq, *j["ham"].ptrs(), pos_lo=lo, pos_hi=hi, anchor=an)
        if i % 3 == 0:
            ctx.reads_edist_anchored_async(ptr, 64, count, k, dq, nq, *j["fixed"].ptrs(), pos_lo=lo, pos_hi=hi)
    ctx.sync()  # the only sync of the queue
    for j in jobs:
        i, count, nq, s, off, queries, (lo, hi) = j["i"], j["count"], j["nq"], j["s"], j["off"], j["queries"], j["rng"]
        anchor = END if j["anchor"] == "end" else START
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, lo, hi)
        got = j["out"].read()
        assert _same(got, want), (i, _diff(got, want))
        ham = j["ham"].read()
        assert _same(ham, rab.reads_anchored_batch(s, off, k, queries, anchor, lo, hi)), i
        assert (got[2] <= ham[2]).all()
        if i % 3 == 0:
            assert _same(j["fixed"].read(), eo.reads_edist(s, 64, count, k, queries, lo, hi)), i


def test_host_forms_above_the_cutoff_in_one_chunk_and_across_two():
    """1,150,000 reads of 100 .. 140 bases, END (0, 3), k = 9, two queries (27.6 * 10^6 span-base-query pairs, above the default cutoff of 2^20) on a
    context with the default dispatch: the ASCII form's first chunk is the longest run of whole reads within 128 Mi bytes, the packed form's within 4 Mi
    words; the reads on both sides of each boundary hold a planted winner.  60,000 reads run in one chunk, 20,000 stay on the host.  Then an N past the
    boundary, inside a span, reports its absolute index; one outside the spans is ignored."""
    import bitnuc_amd as bn
    rng = np.random.default_rng(1283)
    count, k = 1_150_000, 9
    lengths = rng.integers(100, 141, size=count)
    off = rb.offsets_of(lengths)
    wtab = rb.word_offsets_of(off)
    per_ascii = int(np.searchsorted(off, 128 << 20, side="right")) - 1    # the first chunk's reads: the largest r1 with off[r1] <= the budget
    per_packed = int(np.searchsorted(wtab, (128 << 20) // 32, side="right")) - 1
    assert 0 < per_packed < per_ascii < count
    queries = ro.random_queries(rng, 2, k)
    codes = rng.integers(0, 4, size=int(off[-1]), dtype=np.uint8)
    qc = [ro.query_codes(q, k) for q in queries]
    o = off.astype(np.int64)
    for per in (per_ascii, per_packed):
        codes[o[per] - k:o[per]] = qc[0]                                  # the chunk's last read: query 0 in its last k bases
        codes[o[per + 1] - k - 3:o[per + 1] - 3] = qc[1]                  # the next chunk's first read: query 1 at the span's start
        codes[o[per + 2] - k:o[per + 2] - 1] = np.delete(qc[0], 4)        # query 0 with one base deleted
    s = ro.LUT[codes]
    del codes
    want = ebo.reads_edist_batch(s, off, k, queries, END, 0, 3)
    for per in (per_ascii, per_packed):
        ln = [int(lengths[r]) for r in (per - 1, per)]
        assert [_row(want, r)[:3] for r in (per - 1, per)] == [(0, ln[0], 0), (1, ln[1] - 3, 0)] and int(want[2][per + 1]) <= 1
    c = bn.Context(0)
    try:
        got = c.reads_edist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert _same(got, want), _diff(got, want)
        words = rb.pack_batch(s, off)
        got = c.reads_edist_anchored_batch_packed(words, wtab, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert _same(got, want), _diff(got, want)
        got = c.reads_pattern_edist_anchored_batch_packed(words, wtab, off, k, rp.singletons(queries, k), pos_lo=0, pos_hi=3, anchor="end")
        assert _same(got, want), _diff(got, want)
        m, big = 20_000, 60_000  # 480,000 pairs: the host; 1.44 * 10^6 pairs: one chunk through the device
        assert m * 12 * 2 < 1 << 20 <= big * 12 * 2
        assert _same(c.reads_edist_anchored_batch(s, off[:big + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end"), tuple(a[:big] for a in want))
        assert _same(c.reads_edist_anchored_batch_packed(words, wtab[:big + 1], off[:big + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end", second=False),
                     tuple(a[:big] for a in want[:3]))
        assert _same(c.reads_edist_anchored_batch(s, off[:m + 1], k, queries, pos_lo=0, pos_hi=3, anchor="end"), tuple(a[:m] for a in want))  # stays on the host
        s[int(o[per_ascii]) + 7] = ord("N")  # outside the spans: ignored
        assert _same(c.reads_pattern_edist_anchored_batch(s, off, k, rp.singletons(queries, k), pos_lo=0, pos_hi=3, anchor="end"), want)
        bad_at = int(o[per_ascii + 1]) - 9
        s[bad_at] = ord("N")
        with pytest.raises(bn.NucleotideError) as ei:
            c.reads_edist_anchored_batch(s, off, k, queries, pos_lo=0, pos_hi=3, anchor="end")
        assert (ei.value.byte, ei.value.index) == (ord("N"), bad_at)
        del ei
    finally:
        c.close()


def test_cpp_mirror_of_the_ragged_edist_forms(ctx, tmp_path):
    """the four reads_*edist_anchored_batch* methods of include/bitnuc.hpp against the plain DP, via tests/cpp/test_reads_edist_batch_hpp.cpp"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_reads_edist_batch_hpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_reads_edist_batch_hpp.cpp"),
                        "-L", os.path.join(root, "bitnuc_amd"), "-lbitnuc_hip", "-Wl,-rpath," + os.path.join(root, "bitnuc_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_", (33, 64, 150))
def test_identity_with_the_fixed_edist_form_on_equal_lengths(ctx, L_):
    """on the device: START (lo, hi) equals bitnuc_reads_edist_anchored*_async(read_len = L, lo, hi) byte for byte, END (e_lo, e_hi) equals it with
    pos_lo = L - k - e_hi, pos_hi = L - k - e_lo"""
    import torch
    rng = np.random.default_rng(L_)
    count, nq = 200, 7
    off = rb.offsets_of([L_] * count)
    wtab = rb.word_offsets_of(off)
    d_off, d_wtab = _dev_u64(off), _dev_u64(wtab)
    for k in sorted({1, 16, min(31, L_), min(32, L_)}):
        queries = ro.random_queries(rng, nq, k)
        s = ro.random_reads(rng, L_, count, k, queries)
        t, ptr = _ascii_dev(s, 1)
        tw, wptr = _words_dev(ro.pack_reads(s, L_, count), 1)
        dq = _dev_queries(queries)
        last = L_ - k

        def fixed(lo, hi):
            o1, o2 = Out(count), Out(count)
            torch.cuda.synchronize()
            ctx.reads_edist_anchored_async(ptr, L_, count, k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi)
            ctx.reads_edist_anchored_packed_async(wptr, L_, count, k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi)
            return o1.read(ctx), o2.read()

        def ragged(lo, hi, anchor):
            o1, o2 = Out(count), Out(count)
            torch.cuda.synchronize()
            ctx.reads_edist_anchored_batch_async(ptr, d_off, count, int(off[-1]), k, dq, nq, *o1.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            ctx.reads_edist_anchored_batch_packed_async(wptr, d_wtab, d_off, count, int(wtab[-1]), k, dq, nq, *o2.ptrs(), pos_lo=lo, pos_hi=hi, anchor=anchor)
            return o1.read(ctx), o2.read()
        cap = 64 - k
        for lo, hi in ((0, min(3, last)), (last // 2, min(last // 2 + 5, last, last // 2 + cap)), (max(0, last - 3), last), (last, last + min(4, cap))):
            fa, fp = fixed(lo, hi)
            ra_, rp_ = ragged(lo, hi, "start")
            assert _same(ra_, fa) and _same(rp_, fp) and _same(fa, fp), (k, lo, hi)
        for e_lo, e_hi in ((0, 0), (0, min(3, last)), (min(2, last), min(7, last))):
            fa, fp = fixed(last - e_hi, last - e_lo)
            ra_, rp_ = ragged(e_lo, e_hi, "end")
            assert _same(ra_, fa) and _same(rp_, fp), (k, e_lo, e_hi)


def test_never_above_the_ragged_hamming_form(ctx):
    import torch
    rng = np.random.default_rng(0xBEE)
    k, nq, lo, hi = 16, 12, 0, 4
    lengths = _wave_lengths(rng, 300, k, lo, 5)
    queries, s, off = _random(rng, lengths, k, nq, END, lo, hi)
    count = len(lengths)
    want = _check(ctx, s, off, k, queries, END, lo, hi)
    t, ptr = _ascii_dev(s, 0)
    o = Out(count)
    torch.cuda.synchronize()
    ctx.reads_hdist_anchored_batch_async(ptr, _dev_u64(off), count, int(off[-1]), k, _dev_queries(queries), nq, *o.ptrs(), pos_lo=lo, pos_hi=hi, anchor="end")
    ham = o.read(ctx)
    assert (want[2] <= ham[2]).all() and (want[2] < ham[2]).any() and ((want[2] == 0xFF) == (ham[2] == 0xFF)).all()


# ---- 5. the fuzz -----------------------------------------------------------------------------------------------------------------------------
def fuzz_case(rng, it):
    """One case of the differential fuzz: k in [8, 32]; w offsets in [3, min(65 - k, 12)]; pos_lo in [0, 3]; the anchor alternates; up to 300 / 130 / 40 /
    70 reads by the case's class; 1 .. 13 queries.  Half of the reads have the full span (k + pos_lo + w - 1 up to about 100 bases more), a quarter a
    shortened one, an eighth no window (the rest: the full span again); the first three reads are one of each kind.  About 80 % of the reads whose span has
    at least k + 1 bases carry a copy of a query with 1 .. 3 edits, at least one of them an indel, inside the span."""
    k = int(rng.integers(8, 33))
    w = int(rng.integers(3, min(65 - k, 12) + 1))
    lo = int(rng.integers(0, 4))
    anchor = BOTH[it % 2]
    count = int(rng.integers(4, (300, 130, 40, 70)[it % 4]))
    nq = int(rng.integers(1, 14))
    full = k + lo + w - 1
    kinds = rng.choice(3, size=count, p=(0.625, 0.25, 0.125))
    kinds[:3] = (0, 1, 2)
    lengths = np.where(kinds == 0, full + rng.integers(0, 101, size=count),
                       np.where(kinds == 1, k + lo + rng.integers(0, w - 1, size=count), rng.integers(0, k + lo, size=count)))
    queries = ro.random_queries(rng, nq, k)
    off = rb.offsets_of(lengths)
    s = _ascii(rng.integers(0, 4, size=int(off[-1])))
    _plant(rng, s, off, k, queries, anchor, lo, lo + w - 1, share=0.8)
    s[rng.random(s.size) < 0.3] |= 0x20
    return k, w, lo, anchor, queries, s, off


def fuzz_conditions(k, w, lo, anchor, queries, s, off, want):
    """the conditions on a case's inputs, from the oracles alone: among the reads with a window the edit distance is strictly below the ragged Hamming
    oracle's in at least a quarter; the case holds at least one shortened-span read and one read without a window"""
    n = rab.windows(np.diff(off.astype(np.int64)), k, anchor, lo, lo + w - 1)[1]
    ham = rab.reads_anchored_batch(s, off, k, queries, anchor, lo, lo + w - 1)
    has = n > 0
    assert (want[2] <= ham[2]).all() and ((want[2] == 0xFF) == ~has).all()
    below = int((want[2][has] < ham[2][has]).sum())
    assert 4 * below >= int(has.sum()), (k, w, lo, anchor, int(has.sum()), below)
    assert ((n > 0) & (n < w)).any() and (n == 0).any()
    return below / max(1, int(has.sum())), float(((n > 0) & (n < w)).mean()), float((n == 0).mean())


def test_seeded_differential_fuzz(ctx):
    """150 small cases (fuzz_case), each required to hold indels, a shortened span and a read without a window (fuzz_conditions).  On the CPU, for this
    generator and seed: the share of reads with a window whose edit distance is below the Hamming distance is at least 0.27 in every case, the
    shortened-span share at least 0.07 and the no-window share at least 0.02."""
    rng = np.random.default_rng(0xED18)
    for it in range(150):
        k, w, lo, anchor, queries, s, off = fuzz_case(rng, it)
        want = ebo.reads_edist_batch(s, off, k, queries, anchor, lo, lo + w - 1)
        fuzz_conditions(k, w, lo, anchor, queries, s, off, want)
        _check(ctx, s, off, k, queries, anchor, lo, lo + w - 1, want, aoff=int(rng.integers(0, 16)), woff=int(rng.integers(0, 2)),
               tag=(it, k, w, lo, anchor, off.size - 1, len(queries)))
