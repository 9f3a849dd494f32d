"""All 256 byte values in and beside the input of every ASCII-consuming kernel path (-m gpu), through the product library's _dev entry points.

One test per path; a path is the shape and pointer offset that batch_legs / launch_scan / launch_count / launch_hits / launch_count_multi, the codec
launcher and batch.hip route to one kernel (or one kernel + its leftover kernel).  Its input is the smallest at which all its code regions exist --
the head before the first 16-byte aligned base (unaligned pointers), a body round / trip / tile, the halo bytes a round reads for its last windows,
the tail or leftover loop -- derived from the kernels' tiling constants (tests/alphabet.py: KERNEL_CONSTANTS, checked against the sources' text by
tests/test_alphabet_classes.py).  The good sequence stays on the device; a case overwrites one or two bytes, calls, syncs and restores.

Every path asserts
  ACCEPT  the same bases in upper case, lower case and a seeded mix give identical outputs, the oracle's;
  REJECT  alphabet.reject_plan: each of the 248 invalid values once at each byte lane of a dword (992 cases), rotating over the path's regions, comes
          back from the next sync() as InvalidBase(byte, index) with the planted byte and position, which is also what the oracle reports for that
          input; a second invalid byte of the OTHER class planted later in the input (the last base for three lanes of every value, the next base
          for the fourth) never wins; the sync after that is clean (reported once); and
          after the sweep one clean call gives the oracle's result (slot re-armed, tickets and accumulators back at zero);
  IGNORE  for every value b the bytes the entry point does not own -- the 16 before the first base and the 32 after the last one, everything before
          offsets[0] and after offsets[-1] of a ragged batch -- are set to b: the call succeeds with the oracle's result for the unpolluted input and
          the guard bytes around every output stay untouched.  Strided k-mers with k < stride and fixed reads with stride > read_len get one more
          call on ~1100 items whose gap bytes cycle through all 256 values, every value next to a base at every byte lane.
Failures are collected per path and reported together."""
import zlib

import numpy as np
import pytest

import alphabet as ab
import bitnuc_amd as bn

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 256
K = 31
QUERY = 0x9E3779B97F4A7C15  # (its two bits above 2 k are junk the kernels must ignore)
TAU = 23  # just below the mean distance of random 31-mers: about half the windows hit
SCAN_BODY = 6 * ab.ROUND + ab.HALO + 333  # one whole trip of 4 rounds + a partial trip of 2 + the halo + a tail (scan_rounds == 6)


def _torch():
    import torch
    return torch


class Src:
    """The input on the device at byte offset `off` of a 256-byte aligned allocation, 'N' around it; positions are relative to its pointer."""

    def __init__(self, good, off):
        torch = _torch()
        self.n, self.base = int(good.size), PAD + off
        host = np.full(self.base + self.n + PAD, ord("N"), dtype=np.uint8)
        host[self.base:self.base + self.n] = good
        self.clean = torch.from_numpy(host).cuda()
        self.t = self.clean.clone()
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.base

    def load(self, s):
        self.clean[self.base:self.base + self.n] = _torch().from_numpy(np.ascontiguousarray(s)).cuda()
        self.restore()

    def restore(self):
        self.t.copy_(self.clean)

    def poke(self, pos, byte):
        self.t[self.base + pos] = int(byte)


class Out:
    """An output between two guard regions, at byte offset `off` (a multiple of the element size) of a 256-byte aligned allocation."""

    def __init__(self, nbytes, off=0):
        torch = _torch()
        self.n, self.lo = int(nbytes), PAD + off
        self.t = torch.full((self.lo + self.n + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lo

    def reset(self):
        self.t.fill_(GUARD)

    def read(self):
        h = self.t.cpu().numpy()
        return h[self.lo:self.lo + self.n], bool((h[:self.lo] == GUARD).all() and (h[self.lo + self.n:] == GUARD).all())


class Path:
    """good: the input relative to the pointer; regions: [(name, positions)] for reject_plan; launch(ptr) issues the call; want(s) -> the oracle's
    outputs for input s (a prefix of each Out's bytes) or raises OracleError with the index relative to the pointer; owned: the positions the entry
    point examines (default: all); foreign: positions relative to the pointer it must not look at (default: 16 before, 32 after); keep: objects the
    launch needs alive."""

    def __init__(self, name, good, off, regions, outs, launch, want, owned=None, foreign=None, keep=()):
        self.name, self.good, self.regions, self.outs, self.launch, self.want, self.keep = name, good, regions, outs, launch, want, keep
        self.src = Src(good, off)
        self.owned = np.arange(good.size) if owned is None else np.asarray(owned)
        foreign = list(range(-16, 0)) + list(range(good.size, good.size + 32)) if foreign is None else foreign
        self.foreign = _torch().tensor([self.src.base + p for p in foreign], dtype=_torch().int64, device="cuda")
        self.unpolluted = good  # (a gap variant: the same input with plain separators)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def sync_error(ctx):
    try:
        ctx.sync()
        return None
    except bn.NucleotideError as e:
        return (e.kind, getattr(e, "byte", None), getattr(e, "index", None))


def _run(ctx, P):
    _torch().cuda.synchronize()
    P.launch(P.src.ptr)
    return sync_error(ctx)


def _check_outputs(P, want, tag, fails):
    for i, (o, w) in enumerate(zip(P.outs, want)):
        got, intact = o.read()
        wb = np.ascontiguousarray(w).reshape(-1).view(np.uint8)  # (an output of any element size and shape, as bytes)
        if not intact:
            fails.append(tag + f": guard bytes around output {i} overwritten")
        if not np.array_equal(got[:wb.size], wb):
            fails.append(tag + f": output {i} differs from the oracle's at byte {int(np.flatnonzero(got[:wb.size] != wb)[0])}")


def _clean_call(ctx, P, want, tag, fails):
    for o in P.outs:
        o.reset()
    err = _run(ctx, P)
    if err is not None:
        fails.append(tag + f": unexpected error {err}")
    else:
        _check_outputs(P, want, tag, fails)


def run_path(ctx, oracle, P, gap=None):
    fails = []
    want = P.want(P.good)
    # ACCEPT: case does not matter
    not_bases = np.setdiff1d(np.arange(P.good.size), P.owned)
    for case in ("upper", "lower", "mixed"):
        s = ab.recase(P.good, case, 7)
        s[not_bases] = P.good[not_bases]  # separators stay what they are
        P.src.load(s)
        want_s = P.want(s)
        if any(not np.array_equal(a, b) for a, b in zip(want, want_s)):
            fails.append(f"{P.name} accept {case}: the ORACLE's result depends on the case")
        _clean_call(ctx, P, want, f"{P.name} accept {case}", fails)
    # REJECT: every invalid value at every byte lane, over the path's regions
    P.src.load(P.good)
    for case, (byte, pos, region) in enumerate(ab.reject_plan(P.regions)):
        # the second invalid byte: the input's last base (another trip or the tail loop, so the register-level validator alone has to flag the first
        # one's group) for three lanes of every value, the very next base (the rescan has to pick the first of two in one group) for the fourth
        later = P.owned[P.owned > pos]
        near = (case % len(ab.INVALID) + case // len(ab.INVALID)) % 4 == 0
        second = None if later.size == 0 else int(later[0] if near else later[-1])
        s = P.good.copy()
        s[pos] = byte
        P.src.poke(pos, byte)
        if second is not None:
            s[second] = ab.other_class(byte, case)
            P.src.poke(second, s[second])
        got = _run(ctx, P)
        again = sync_error(ctx)
        P.src.restore()
        try:
            P.want(s)
            orc = None
        except oracle.OracleError as e:
            orc = (e.kind, e.byte, e.index)
        tag = f"{P.name} reject {ab.describe(byte)} at {pos} (lane {pos % 4}, {pos % 16} mod 16, region {region!r}), second invalid byte at {second}"
        if got != ("InvalidBase", byte, pos) or orc != ("InvalidBase", byte, pos):
            fails.append(tag + f": error {got}, oracle {orc}")
        if again is not None:
            fails.append(tag + f": reported again by the next sync: {again}")
    _clean_call(ctx, P, want, f"{P.name} clean call after the sweep", fails)
    # IGNORE: the bytes around the input take every value
    for b in range(256):
        P.src.t[P.foreign] = b
        _clean_call(ctx, P, want, f"{P.name} ignore 0x{b:02X} around the input", fails)
    P.src.restore()
    if gap is not None:
        _clean_call(ctx, gap, gap.want(gap.unpolluted), f"{gap.name} gap bytes of every value", fails)
    assert not fails, "\n".join(fails[:25]) + f"\n({len(fails)} failing checks)"


def _head(off):
    return (16 - off) % 16


# ---- the bulk codec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 5], ids=["encode_kernel-aligned", "encode_kernel-src+5"])
def test_encode(ctx, oracle, off):
    """one whole workgroup tile, five leftover 16-byte groups (encode_tail's loop) and 11 last bases (its byte loop)"""
    name = f"encode_dev src+{off}"
    n = ab.ENCODE_TILE + 5 * ab.GROUP + 11
    h, groups_end = _head(off), n - n % ab.GROUP
    regions = ([("head", range(0, h))] if h else []) + [("tile", range(h, ab.ENCODE_TILE)), ("leftover groups", range(ab.ENCODE_TILE, groups_end)),
                                                         ("last bases", range(groups_end, n))]
    out = Out(8 * ((n + 31) // 32))
    P = Path(name, ab.bases(_rng(name), n), off, regions, [out], lambda ptr: ctx.encode_dev(ptr, n, out.ptr), lambda s: [oracle.encode(s)])
    run_path(ctx, oracle, P)


# ---- k-mer batches -------------------------------------------------------------------------------------------------------------------
def batch_regions(k, stride, count, off, out_off):
    """The code regions of one as_2bit_batch_dev call, as kmer.hip's batch_legs routes it -> (kernels, [(region, positions)])."""
    span = (count - 1) * stride + k
    owned = np.arange(span)
    if stride > k:
        owned = owned[owned % stride < k]

    def within(lo, hi):
        return owned[(owned >= lo) & (owned < hi)]
    al, oal, h = off % 16 == 0, out_off % 16 == 0, _head(off)
    if stride == k and count >= 64:
        items = count // 64
        dense_end, regs = items * 64 * k, [("head", within(0, h))] if h else []
        if items >= 3 and not h:
            regs += [("first item", within(0, 64 * k)), ("middle items", within(64 * k, dense_end - 64 * k)), ("last item", within(dense_end - 64 * k, dense_end))]
        else:
            regs += [("dense items", within(h, dense_end))]
        if items * 64 < count:
            regs += [("leftover k-mers", within(dense_end, span))]
        return "kmer_dense_kernel" + ("" if items * 64 == count else " + kmer_batch_kernel<true>"), regs
    if stride == 1 and al and oal and span >= ab.ROUND + ab.HALO:
        r = ab.scan_rounds(span)
        trip = min(r, ab.TRIP) * ab.ROUND
        regs = [("first trip", within(0, trip))] + ([("later rounds", within(trip, r * ab.ROUND))] if r > ab.TRIP else [])
        return "kmer_slide2_kernel + kmer_batch_kernel<true>", regs + [("halo", within(r * ab.ROUND, r * ab.ROUND + ab.HALO)), ("leftover", within(r * ab.ROUND + ab.HALO, span))]
    slide = stride in (1, 2, 4, 8, 16) and k >= stride and al and oal and span >= ab.ROUND
    slide_any = not slide and 3 <= stride < 32 and k >= stride and al and span >= ab.ROUND
    if slide or slide_any:
        r = ab.rounds992(span)
        body, read_end = r * ab.ROUND992, (r - 1) * ab.ROUND992 + ab.ROUND
        return (f"kmer_slide_kernel<{stride}>" if slide else "kmer_slide_any_kernel") + " + kmer_batch_kernel<true>", [
            ("rounds", within(0, body)), ("halo", within(body, read_end)), ("leftover", within(read_end, span))]
    blk = ab.KERNEL_CONSTANTS["kBlock"][0]
    last = (count - 1) // blk * blk
    staged = stride <= ab.KERNEL_CONSTANTS["kStagedMaxStride"][0]
    return f"kmer_batch_kernel<{'true' if staged else 'false'}>", [("first block", within(0, blk * stride)), ("middle blocks", within(blk * stride, last * stride)),
                                                                    ("last block", within(last * stride, span))]


# name: (k, stride, count, src offset, output offset, the kernels batch_legs launches)
BATCH_SHAPES = {
    "dense-aligned": (K, K, 192, 0, 0, "kmer_dense_kernel"),
    "dense-src+1-leftover": (K, K, 2 * 64 + 37, 1, 0, "kmer_dense_kernel + kmer_batch_kernel<true>"),
    "stride1-slide2": (K, 1, SCAN_BODY - K + 1, 0, 0, "kmer_slide2_kernel + kmer_batch_kernel<true>"),
    "stride1-below-1056": (K, 1, 1050 - K + 1, 0, 0, "kmer_slide_kernel<1> + kmer_batch_kernel<true>"),
    "stride2": (K, 2, (2300 - K) // 2 + 1, 0, 0, "kmer_slide_kernel<2> + kmer_batch_kernel<true>"),
    "stride4": (K, 4, (2300 - K) // 4 + 1, 0, 0, "kmer_slide_kernel<4> + kmer_batch_kernel<true>"),
    "stride8": (K, 8, (2300 - K) // 8 + 1, 0, 0, "kmer_slide_kernel<8> + kmer_batch_kernel<true>"),
    "stride16": (K, 16, (2300 - K) // 16 + 1, 0, 0, "kmer_slide_kernel<16> + kmer_batch_kernel<true>"),
    "stride5-any": (K, 5, (2300 - K) // 5 + 1, 0, 0, "kmer_slide_any_kernel + kmer_batch_kernel<true>"),
    "stride24-any": (K, 24, (2300 - K) // 24 + 1, 0, 0, "kmer_slide_any_kernel + kmer_batch_kernel<true>"),
    "stride1-out-8-mod-16": (K, 1, 1200, 0, 8, "kmer_batch_kernel<true>"),  # (1230 bytes: only the output's alignment keeps it off the sliding kernels)
    "gaps-staged": (21, 41, 600, 3, 0, "kmer_batch_kernel<true>"),
    "gaps-unstaged": (K, 71, 600, 0, 0, "kmer_batch_kernel<false>"),
}
GAP_ITEMS = 1100  # item j's gap bytes hold (j // 4) mod 256 and the strides are odd: every value next to a base at every byte lane


def gap_fill(s, unit, stride, count):
    """the bytes between the items (unit bytes every stride) take item j's value (j // 4) mod 256 -> s; checks the coverage it promises"""
    assert stride % 2 == 1 and count >= 1024 + 4
    pos = np.arange(s.size)
    gap = pos % stride >= unit
    s[gap] = ((pos[gap] // stride) // 4) % 256
    for edge in (unit, stride - 1):  # the gap byte right after an item's last base, the one right before the next item's first base
        p = np.arange(count - 1) * stride + edge
        assert len({(int(v), int(q % 4)) for v, q in zip(s[p], p)}) == 1024
    return s


def batch_path(ctx, oracle, shape, count=None, gaps=False):
    k, stride, n_items, off, out_off, _ = BATCH_SHAPES[shape]
    count = n_items if count is None else count
    name = f"as_2bit_batch_dev {shape} (k={k} stride={stride} count={count} src+{off} out+{out_off})"
    span = (count - 1) * stride + k
    good = ab.bases(_rng(name), span)
    if stride > k:
        good[np.arange(span) % stride >= k] = ord("\n")
    _, regions = batch_regions(k, stride, count, off, out_off)
    out = Out(8 * count, out_off)
    owned = np.arange(span)[np.arange(span) % stride < k] if stride > k else None
    P = Path(name, gap_fill(good.copy(), k, stride, count) if gaps else good, off, regions, [out], lambda ptr: ctx.as_2bit_batch_dev(ptr, k, stride, count, out.ptr),
             lambda s: [oracle.as_2bit_batch(s, k, stride, count)], owned=owned)
    P.unpolluted = good
    return P


@pytest.mark.parametrize("shape", list(BATCH_SHAPES))
def test_kmer_batch(ctx, oracle, shape):
    k, stride, count, off, out_off, kernels = BATCH_SHAPES[shape]
    assert batch_regions(k, stride, count, off, out_off)[0] == kernels  # the routing the shape was chosen for
    P = batch_path(ctx, oracle, shape)
    run_path(ctx, oracle, P, gap=batch_path(ctx, oracle, shape, GAP_ITEMS, gaps=True) if stride > k else None)


# ---- the scan, its counts and hit lists ----------------------------------------------------------------------------------------------------
def scan_regions(n, off, rounds_from_skip, r992=False):
    """head: the bytes before the first 16-byte aligned base; rounds; the halo the last round reads; the tail loop.  rounds_from_skip: the rounds
    start at the first aligned base (hit lists, multi-query count), else at the pointer (the unaligned scan and count load unaligned groups)."""
    h = _head(off)
    start = h if rounds_from_skip else 0
    if r992:
        r = ab.rounds992(n)
        body, read_end = r * ab.ROUND992, (r - 1) * ab.ROUND992 + ab.ROUND
    else:
        r = ab.scan_rounds(n, start)
        body, read_end = start + r * ab.ROUND, start + r * ab.ROUND + ab.HALO
    assert r > ab.TRIP and r % ab.TRIP  # one whole trip and a partial one
    return ([("head", range(0, h))] if h else []) + [("rounds", range(h, body)), ("halo", range(body, read_end)), ("tail", range(read_end, n))]


@pytest.mark.parametrize("off", [0, 3], ids=["kmer_scan_seg_mfma_kernel-aligned", "kmer_scan_kernel-ref+3"])
def test_scan(ctx, oracle, off):
    name = f"kmer_hdist_scan_dev ref+{off}"
    n = _head(off) + SCAN_BODY
    out = Out(n - K + 1)
    P = Path(name, ab.bases(_rng(name), n), off, scan_regions(n, off, False, r992=off != 0), [out],
             lambda ptr: ctx.kmer_hdist_scan_dev(ptr, n, K, QUERY, out.ptr), lambda s: [oracle.kmer_hdist_scan(s, K, QUERY)])
    run_path(ctx, oracle, P)


@pytest.mark.parametrize("off", [0, 7], ids=["kmer_count3_mfma_kernel-aligned", "kmer_scan2_kernel-ref+7"])
def test_count(ctx, oracle, off):
    name = f"kmer_hdist_count_dev ref+{off}"
    n = _head(off) + SCAN_BODY
    out = Out(8)
    P = Path(name, ab.bases(_rng(name), n), off, scan_regions(n, off, False), [out], lambda ptr: ctx.kmer_hdist_count_dev(ptr, n, K, QUERY, TAU, out.ptr),
             lambda s: [np.array([int((oracle.kmer_hdist_scan(s, K, QUERY) <= TAU).sum())], dtype=np.uint64)])
    run_path(ctx, oracle, P)


@pytest.mark.parametrize("capped", [False, True], ids=["cap0", "capped"])
@pytest.mark.parametrize("off", [0, 9], ids=["ref+0", "ref+9"])
def test_hits(ctx, oracle, off, capped):
    """kmer_hits_mfma_kernel<false> latches (the count pass); with a cap the emit pass kmer_hits_mfma_kernel<true> runs behind it"""
    name = f"kmer_hdist_hits_dev ref+{off} {'capped' if capped else 'cap 0'}"
    n = _head(off) + SCAN_BODY
    good = ab.bases(_rng(name), n)
    total = int((oracle.kmer_hdist_scan(good, K, QUERY) <= TAU).sum())
    assert total > 30
    cap = total // 3 if capped else 0
    pos, hd, nh = Out(8 * cap), Out(cap, 3), Out(8, 8)

    def want(s):
        d = oracle.kmer_hdist_scan(s, K, QUERY)
        hits = np.flatnonzero(d <= TAU)
        g = min(cap, hits.size)
        return [hits[:g].astype(np.uint64), d[hits[:g]], np.array([hits.size], dtype=np.uint64)]
    P = Path(name, good, off, scan_regions(n, off, True), [pos, hd, nh],
             lambda ptr: ctx.kmer_hdist_hits_dev(ptr, n, K, QUERY, TAU, pos.ptr, hd.ptr, cap, nh.ptr), want)
    run_path(ctx, oracle, P)


@pytest.mark.parametrize("nq", [1, 17], ids=["1query", "17queries"])
@pytest.mark.parametrize("off", [0, 9], ids=["ref+0", "ref+9"])
def test_count_multi(ctx, oracle, off, nq):
    """17 queries are two query blocks (kMultiQB = 16): both see the invalid byte, one reports it"""
    torch = _torch()
    name = f"kmer_hdist_count_multi_dev ref+{off} {nq} queries"
    n = _head(off) + SCAN_BODY
    rng = _rng(name)
    distinct = [QUERY, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62))]
    queries = np.array([distinct[i % 3] for i in range(nq)], dtype=np.uint64)
    taus = np.array([(TAU, TAU - 2, TAU + 1, K, 0)[i % 5] for i in range(nq)], dtype=np.uint32)
    dq, dt = torch.from_numpy(queries.view(np.int64)).cuda(), torch.from_numpy(taus.view(np.int32)).cuda()
    out = Out(8 * nq)

    def want(s):
        d = [oracle.kmer_hdist_scan(s, K, q) for q in distinct]
        return [np.array([int((d[i % 3] <= int(taus[i])).sum()) for i in range(nq)], dtype=np.uint64)]
    P = Path(name, ab.bases(rng, n), off, scan_regions(n, off, True), [out],
             lambda ptr: ctx.kmer_hdist_count_multi_dev(ptr, n, K, dq, dt, nq, out.ptr), want, keep=(dq, dt))
    run_path(ctx, oracle, P)
    assert np.array_equal(dq.cpu().numpy().view(np.uint64), queries) and np.array_equal(dt.cpu().numpy().view(np.uint32), taus)


# ---- read batches --------------------------------------------------------------------------------------------------------------------
def _encode_reads(oracle, s, bounds):
    """the oracle's words of the reads [lo, hi) of s, back to back; an invalid byte is reported at its index in s"""
    words = []
    for lo, hi in bounds:
        if hi > lo:
            try:
                words.append(oracle.encode(s[lo:hi]))
            except oracle.OracleError as e:
                e.index += lo
                raise
    return [np.concatenate(words)]


RAGGED_LENS = (37, 150, 0, 31, 32, 33, 1, 64, 100, 2500, 151, 16, 150, 29)  # mixed lengths, an empty read, one read of 79 words (more than a 64-word tile)
RAGGED_FIRST = 21                                                           # offsets[0]: not a multiple of 16


@pytest.mark.parametrize("via", ["plan", "tables"])
def test_ragged_batch(ctx, oracle, via):
    """encode_batch_plan_kernel behind BatchPlan.encode_dev and behind the table-driven encode_batch_dev"""
    torch = _torch()
    name = f"ragged batch via {via}"
    off = np.zeros(len(RAGGED_LENS) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(RAGGED_LENS)
    off += np.uint64(RAGGED_FIRST)
    end, count = int(off[-1]), len(RAGGED_LENS)
    bounds = [(int(off[i]), int(off[i + 1])) for i in range(count)]
    good = ab.bases(_rng(name), end)
    good[:RAGGED_FIRST] = ord("N")  # before offsets[0]: not the batch's
    long_lo, long_hi = bounds[RAGGED_LENS.index(2500)]
    regions = [("first chunk", range(RAGGED_FIRST, 32)), ("short reads", range(32, long_lo)), ("the long read", range(long_lo, long_hi)),
               ("last reads", range(long_hi, end))]
    tw = int(sum((x + 31) // 32 for x in RAGGED_LENS))
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_wo = torch.zeros(count + 1, dtype=torch.int64, device="cuda")
    assert ctx.batch_word_offsets_dev(d_off, count, d_wo) == tw
    plan = bn.BatchPlan(ctx, d_off, count)
    assert plan.total_words == tw
    out = Out(8 * tw)
    if via == "plan":
        launch = lambda ptr: plan.encode_dev(ptr, out.ptr)  # noqa: E731
    else:
        launch = lambda ptr: ctx.encode_batch_dev(ptr, d_off, d_wo, count, tw, out.ptr)  # noqa: E731
    P = Path(name, good, 0, regions, [out], launch, lambda s: _encode_reads(oracle, s, bounds), owned=np.arange(RAGGED_FIRST, end),
             foreign=list(range(-16, RAGGED_FIRST)) + list(range(end, end + 32)), keep=(d_off, d_wo, plan))
    try:
        run_path(ctx, oracle, P)
    finally:
        plan.close()


READ_LEN, READS = 150, 100  # 5 words per read: 12.8 reads per 64-word tile, 8 tiles


def fixed_path(ctx, oracle, stride, off, count=READS, gaps=False):
    name = f"encode_fixed_dev read_len={READ_LEN} stride={stride} count={count} src+{off}"
    n = (count - 1) * stride + READ_LEN
    good = ab.bases(_rng(name), n)
    owned = np.arange(n)[np.arange(n) % stride < READ_LEN]
    if stride > READ_LEN:
        good[np.arange(n) % stride >= READ_LEN] = ord("\n")
    bounds = [(r * stride, r * stride + READ_LEN) for r in range(count)]
    wpr = (READ_LEN + 31) // 32
    tile_reads = ab.TILE_WORDS // wpr  # the reads that lie wholly in the first tile
    regions = [("first tile", owned[owned < tile_reads * stride]), ("middle tiles", owned[(owned >= tile_reads * stride) & (owned < (count - 1) * stride)]),
               ("last read", owned[owned >= (count - 1) * stride])]
    out = Out(8 * wpr * count)
    P = Path(name, gap_fill(good.copy(), READ_LEN, stride, count) if gaps else good, off, regions, [out],
             lambda ptr: ctx.encode_fixed_dev(ptr, READ_LEN, stride, count, out.ptr), lambda s: _encode_reads(oracle, s, bounds), owned=owned)
    P.unpolluted = good
    return P


@pytest.mark.parametrize("stride,off", [(READ_LEN, 6), (READ_LEN + 3, 9)], ids=["back-to-back-src+6", "stride+3-src+9"])
def test_fixed_reads(ctx, oracle, stride, off):
    P = fixed_path(ctx, oracle, stride, off)
    run_path(ctx, oracle, P, gap=fixed_path(ctx, oracle, stride, off, GAP_ITEMS, gaps=True) if stride > READ_LEN else None)
