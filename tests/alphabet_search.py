"""The shapes, owned and foreign bytes, code regions and expected values of tests/test_gpu_alphabet_search.py (no GPU, no library;
tests/test_alphabet_classes.py checks every plan here on the CPU).

One Spec per ASCII kernel path of the search entry points that came after tests/test_gpu_alphabet.py: along a reference (Hamming best match and
histogram, pattern hit list and count, edit-distance best match, count and hit list) and per read (Hamming best match, runner-up and ragged batch;
the anchored matchers on fixed and ragged batches under Hamming distance, edit distance and patterns; the whole-read edit-distance matchers).

  owned     the positions (relative to the pointer, ascending) whose bytes the entry point validates, written from the validation paragraph of its
            block in include/bitnuc_hip.h, never from a kernel: all n bytes along a reference and for the whole-read Hamming forms; the span bytes
            [pos_lo, hi_eff + k) of every read for the anchored forms (ragged: a_r .. a_r + n_r + k - 1 by reads_anchored_batch_oracle.windows, the
            header's definition of the admissible offsets); every byte of the reads of at least k bases for the ragged whole-read edit distance.
  foreign   the positions it must never examine: every other byte of the batch, the 16 before the pointer and the 32 after the last byte.
  regions   at most four code regions of the path's kernel that partition `owned`, each with a position at every byte lane, from the tiling
            constants in alphabet.KERNEL_CONSTANTS.
  want      the expected outputs from the family oracles in tests/; an input with an invalid byte at an owned position raises oracle.OracleError for
            the FIRST such byte in buffer order, whatever the foreign bytes hold.

The ragged tables start at 0, as the header requires of them ("offsets[0] == 0 (a batch cut out of a larger table passes a rebased table)"): the bytes
in front of the batch are the 16 before the pointer."""
import zlib
from types import SimpleNamespace

import numpy as np

import alphabet as ab
import hist_oracle as ho
import kmer_edist_hits_oracle as kh
import kmer_edist_oracle as ko
import pattern_oracle as po
import reads_anchored_batch_oracle as rab
import reads_anchored_oracle as ra
import reads_batch_oracle as rb
import reads_best2_oracle as r2
import reads_best_oracle as ro
import reads_edist_batch_oracle as eb
import reads_edist_best_oracle as ebo
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

KC = {k: v for k, (v, _) in ab.KERNEL_CONSTANTS.items()}
ANCHOR_MAX_SPAN = 64  # BITNUC_ANCHOR_MAX_SPAN (test_alphabet_classes.py reads it back from the header)
WAVE = 32 * KC["kAnchorGroups"]  # reads per wave of the per-read kernels: kAnchorGroups groups of 32 (anchored), one read per lane (edit distance)
PIECE = 8             # bytes per piece of anchored_piece_ascii
EDIST_PIECE = 64      # bases per piece of the whole-read edit-distance kernels (EdistCols' 64 steps per load)
K = 31
QUERY = 0x9E3779B97F4A7C15
SCAN_BODY = 6 * ab.ROUND + ab.HALO + 333  # tests/test_gpu_alphabet.py's: one whole trip of four rounds, a partial trip of two, the halo, a tail
EDIST_REF_N = 2 * KC["kEdistRefChunk"] + KC["kEdistRefLead"] + 37  # two whole chunks and a partial third, its last trip partial
VALID = np.array(ab.VALID, dtype=np.uint8)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def head(off):
    return (16 - off) % 16


class Spec:
    """good: the input relative to the pointer (at byte offset `off` of an aligned allocation); inputs: {name: array} the call reads from device
    memory besides it; outs: [(bytes, byte offset)] one per output; call(ctx, ptr, d, o): issues the entry point with the device addresses d[name]
    and o[i]; compute(oracle, s) -> the expected bytes of every output for a valid input s."""

    def __init__(self, name, good, off, regions, outs, call, compute, inputs=None, owned=None, foreign=None):
        self.name, self.good, self.off, self.outs, self.call, self.compute = name, good, off, outs, call, compute
        self.inputs = inputs or {}
        n = good.size
        self.owned = np.arange(n) if owned is None else np.asarray(owned, dtype=np.int64)
        inside = np.setdiff1d(np.arange(n), self.owned)
        self.foreign = list(range(-16, 0)) + [int(p) for p in inside] + list(range(n, n + 32)) if foreign is None else foreign
        self.regions = [(nm, np.asarray(list(p), dtype=np.int64)) for nm, p in regions]
        self.unpolluted = good

    def want(self, oracle, s):
        v = s[self.owned]
        bad = np.flatnonzero(~np.isin(v, VALID))
        if bad.size:
            raise oracle.OracleError(SimpleNamespace(status=1, byte=int(v[bad[0]]), value=0, index=int(self.owned[bad[0]])))
        return [np.ascontiguousarray(a).reshape(-1) for a in self.compute(oracle, s)]


def gap_fill(spec):
    """The foreign bytes inside the batch take every value: the byte directly behind an owned range and the byte directly in front of one walk
    through 0 .. 255 once per byte lane, the others get a value from their position -> spec with the polluted input, the clean one as .unpolluted.
    Checks that every value then stands directly before and directly after an owned range at every byte lane."""
    good, o = spec.good, spec.owned
    is_owned = np.zeros(good.size, dtype=bool)
    is_owned[o] = True
    starts = o[np.flatnonzero(np.diff(o, prepend=-2) > 1)]
    ends = o[np.flatnonzero(np.diff(o, append=good.size + 1) > 1)] + 1
    inside = np.flatnonzero(~is_owned)
    s = good.copy()
    s[inside] = (inside * 7 + 3) % 256
    edges = (ends[ends < good.size], starts[starts > 0] - 1)
    for edge in edges:
        seen = [0, 0, 0, 0]
        for p in edge:
            s[p] = seen[p % 4] % 256
            seen[p % 4] += 1
    for edge in edges:
        assert not is_owned[edge].any() and len({(int(v), int(p % 4)) for v, p in zip(s[edge], edge)}) == 1024, (spec.name, "gap coverage")
    spec.good, spec.unpolluted = s, good
    return spec


# ---- along a reference: the rounds of 1024 start at the first 16-byte aligned base ------------------------------------------------------------
def scan_regions(n, off):
    """head: the bytes before the first aligned base (the one-window path in front of `skip`); first trip: the rounds 0 .. 3; later rounds: the
    partial trip; the halo the last round reads for its last windows and the tail windows behind it (one region where a head exists)"""
    h = head(off)
    r = ab.scan_rounds(n, h)
    assert r > ab.TRIP and r % ab.TRIP  # one whole trip and a partial one
    trip, body = h + ab.TRIP * ab.ROUND, h + r * ab.ROUND
    regs = ([("head", range(0, h))] if h else []) + [("first trip", range(h, trip)), ("later rounds", range(trip, body))]
    if h:
        return regs + [("halo and tail windows", range(body, n))]
    return regs + [("halo", range(body, body + ab.HALO)), ("tail windows", range(body + ab.HALO, n))]


REF_OFFS = (0, 11)
Q17 = 17  # two query blocks (kMultiQB = 16): only block 0 may latch


def _queries17(rng):
    distinct = [QUERY, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62))]
    return distinct, np.array([distinct[i % 3] for i in range(Q17)], dtype=np.uint64)


def kmer_hdist_best(off):
    name = f"kmer_hdist_best_async ref+{off}"
    rng = rng_of(name)
    n = head(off) + SCAN_BODY
    distinct, queries = _queries17(rng)

    def compute(oracle, s):
        d = [oracle.kmer_hdist_scan(s, K, q) for q in distinct]
        return [np.array([int(np.argmin(d[i % 3])) for i in range(Q17)], dtype=np.uint64), np.array([int(d[i % 3].min()) for i in range(Q17)], dtype=np.uint8)]
    return Spec(name, ab.bases(rng, n), off, scan_regions(n, off), [(8 * Q17, 0), (Q17, 3)],
                lambda ctx, ptr, d, o: ctx.kmer_hdist_best_async(ptr, n, K, d["queries"], Q17, o[0], o[1]), compute, {"queries": queries})


HIST_K = 12  # random 12-mers: the bins below 8 are not empty


def kmer_hdist_hist(off, n_bins):
    name = f"kmer_hdist_hist_async ref+{off} n_bins={n_bins} ({'one tier' if n_bins <= 8 else 'two tiers'})"
    rng = rng_of(name)
    n = head(off) + SCAN_BODY
    distinct, queries = _queries17(rng)

    def compute(oracle, s):
        h = ho.hist(oracle, s, HIST_K, distinct, n_bins)
        return [h[np.arange(Q17) % 3]]
    return Spec(name, ab.bases(rng, n), off, scan_regions(n, off), [(8 * Q17 * n_bins, 0)],
                lambda ctx, ptr, d, o: ctx.kmer_hdist_hist_async(ptr, n, HIST_K, d["queries"], Q17, n_bins, o[0]), compute, {"queries": queries})


def _pattern_with_n(query, k, at=(3, 17, 30)):
    sets = [{0, 1, 2, 3} if i in at else {(int(query) >> (2 * i)) & 3} for i in range(k)]
    return po.from_sets(sets)


PATTERN_TAU = 21


def kmer_pattern_hits(off, capped):
    name = f"kmer_pattern_hits_async ref+{off} {'capped' if capped else 'cap 0'}"
    rng = rng_of(name)
    n = head(off) + SCAN_BODY
    good = ab.bases(rng, n)
    pat = _pattern_with_n(QUERY, K)
    total = po.count(po.pdist(po.codes_of_ascii(good), pat, K), PATTERN_TAU)
    assert total > 30
    cap = total // 3 if capped else 0

    def compute(oracle, s):
        pos, dist, tot = po.hits(po.pdist(po.codes_of_ascii(s), pat, K), PATTERN_TAU, cap)
        return [pos, dist, np.array([tot], dtype=np.uint64)]
    return Spec(name, good, off, scan_regions(n, off), [(8 * cap, 0), (cap, 3), (8, 8)],
                lambda ctx, ptr, d, o: ctx.kmer_pattern_hits_async(ptr, n, K, pat, PATTERN_TAU, o[0], o[1], cap, o[2]), compute)


def kmer_pattern_count_multi(off):
    name = f"kmer_pattern_count_multi_async ref+{off}"
    rng = rng_of(name)
    n = head(off) + SCAN_BODY
    pats = np.stack([_pattern_with_n(QUERY, K), _pattern_with_n(int(rng.integers(0, 1 << 62)), K, (0, 15)), po.from_2bit(int(rng.integers(0, 1 << 62)), K)])
    taus = np.array([PATTERN_TAU, PATTERN_TAU - 2, K], dtype=np.uint32)

    def compute(oracle, s):
        codes = po.codes_of_ascii(s)
        return [np.array([po.count(po.pdist(codes, p, K), int(t)) for p, t in zip(pats, taus)], dtype=np.uint64)]
    return Spec(name, ab.bases(rng, n), off, scan_regions(n, off), [(8 * 3, 0)],
                lambda ctx, ptr, d, o: ctx.kmer_pattern_count_multi_async(ptr, n, K, d["patterns"], d["taus"], 3, o[0]), compute,
                {"patterns": pats, "taus": taus})


# ---- edit distance along a reference: chunks of 1024 columns from the pointer, one per lane --------------------------------------------------
EDIST_REF_OFFS = (0, 5)
EK = 16
Q5 = KC["kEdistInterleave"] + 1  # kEdistInterleave = 4: a group of four queries and a group of one; only the first group's walk may latch


def edist_ref_regions(n):
    """the first chunk (no lead-in) up to the columns the second chunk's lane reads too; the kEdistRefLead columns in front of every chunk boundary,
    which two lanes read; the chunk bodies; the buffer's last trip, which is partial and loads byte by byte"""
    c, lead, trip = KC["kEdistRefChunk"], KC["kEdistRefLead"], KC["kEdistRefTrip"]
    assert n > 2 * c + lead and n % trip  # two whole chunks, a third with a whole trip, and a partial last trip
    pos = np.arange(n)
    last_trip = n - n % trip
    is_lead = (pos >= c - lead) & (pos % c >= c - lead) & (pos < (n // c) * c)
    return [("first chunk", pos[(pos < c) & ~is_lead]), ("lead-in columns two lanes read", pos[is_lead]),
            ("chunk body", pos[(pos >= c) & ~is_lead & (pos < last_trip)]), ("last partial trip", pos[pos >= last_trip])]


def _edist_queries(rng):
    return ro.random_queries(rng, Q5, EK)


def kmer_edist_best(off):
    name = f"kmer_edist_best_async ref+{off}"
    rng = rng_of(name)
    n = EDIST_REF_N
    queries = _edist_queries(rng)
    return Spec(name, ab.bases(rng, n), off, edist_ref_regions(n), [(8 * Q5, 0), (Q5, 3)],
                lambda ctx, ptr, d, o: ctx.kmer_edist_best_async(ptr, n, EK, d["queries"], Q5, o[0], o[1]),
                lambda oracle, s: list(ko.kmer_edist_best(ro.codes_of(s), EK, ko.singletons(queries, EK))), {"queries": queries})


def kmer_edist_count_multi(off):
    name = f"kmer_edist_count_multi_async ref+{off}"
    rng = rng_of(name)
    n = EDIST_REF_N
    queries = _edist_queries(rng)
    taus = np.array([6, 7, 8, EK, 0], dtype=np.uint32)
    return Spec(name, ab.bases(rng, n), off, edist_ref_regions(n), [(8 * Q5, 0)],
                lambda ctx, ptr, d, o: ctx.kmer_edist_count_multi_async(ptr, n, EK, d["queries"], d["taus"], Q5, o[0]),
                lambda oracle, s: [ko.kmer_edist_count(ro.codes_of(s), EK, ko.singletons(queries, EK), taus)], {"queries": queries, "taus": taus})


EDIST_HITS_TAU = 2


def kmer_edist_hits(off, above, with_dist):
    """copies of the query in the first and in the third chunk, none in the second: the emit pass walks two chunks and skips one"""
    name = f"kmer_edist_hits_async ref+{off} cap {'above' if above else 'below'} n_hits, {'with' if with_dist else 'without'} hit_dist"
    rng = rng_of(f"kmer_edist_hits_async ref+{off}")
    n, c = EDIST_REF_N, KC["kEdistRefChunk"]
    query = int(ro.random_queries(rng, 1, EK)[0])
    qc = ro.query_codes(query, EK)
    codes = rng.integers(0, 4, size=n)
    codes[300:300 + EK - 1] = np.delete(qc, 5)       # one base deleted, in the first chunk
    codes[2100:2100 + EK] = qc                        # an exact copy that ends in the last partial trip
    good = ab.recase(ro.LUT[codes].astype(np.uint8), "mixed", off)
    pat = po.from_2bit(query, EK)
    ends, _ = kh.hits(ro.codes_of(good), EK, pat, EDIST_HITS_TAU)
    chunks = {int(j - 1) // c for j in ends}
    assert chunks == {0, 2} and ends.size >= 4, (chunks, ends)
    cap = ends.size + 3 if above else ends.size // 2

    def compute(oracle, s):
        e, d = kh.hits(ro.codes_of(s), EK, pat, EDIST_HITS_TAU)
        g = min(cap, e.size)
        return [e[:g]] + ([d[:g]] if with_dist else []) + [np.array([e.size], dtype=np.uint64)]
    outs = [(8 * cap, 0)] + ([(cap, 3)] if with_dist else []) + [(8, 8)]
    return Spec(name, good, off, edist_ref_regions(n), outs,
                lambda ctx, ptr, d, o: ctx.kmer_edist_hits_async(ptr, n, EK, query, EDIST_HITS_TAU, o[0], o[1] if with_dist else None, cap, o[-1]), compute)


# ---- per read, the whole read, Hamming: the reference kernels' rounds over count * read_len bases ---------------------------------------------
RK = 21


def _thirds(n, edge=256):
    return [("the first 256 windows", range(0, edge)), ("the middle", range(edge, n - edge)), ("the last 256 windows", range(n - edge, n))]


def reads_hdist_best(read_len, count, off, k=RK, second=False):
    fn = "reads_hdist_best2_async" if second else "reads_hdist_best_async"
    name = f"{fn} {read_len} x {count} reads+{off}"
    rng = rng_of(name)
    n = read_len * count
    _, queries = _queries17(rng)
    if read_len >= KC["kReadsMinPeriod"]:
        regions = scan_regions(n, off)
    else:
        assert ab.scan_rounds(n, head(off)) > 0  # long enough for rounds: only the period keeps it on the one-window-per-thread path
        regions = _thirds(n)
    if second:
        return Spec(name, ab.bases(rng, n), off, regions, [(4 * count, 0), (4 * count, 4), (count, 1)] * 2,
                    lambda ctx, ptr, d, o: ctx.reads_hdist_best2_async(ptr, read_len, count, k, d["queries"], Q17, *o),
                    lambda oracle, s: list(r2.reads_best2(s, read_len, count, k, queries)), {"queries": queries})
    return Spec(name, ab.bases(rng, n), off, regions, [(4 * count, 0), (4 * count, 4), (count, 1)],
                lambda ctx, ptr, d, o: ctx.reads_hdist_best_async(ptr, read_len, count, k, d["queries"], Q17, *o),
                lambda oracle, s: list(ro.reads_best(s, read_len, count, k, queries)), {"queries": queries})


def reads_hdist_best_batch(off=5, k=RK):
    """an empty read, k - 1, k, 31, 32 and 33 bases (the first round touches reads of 1 .. 31 bases: the exact path), then reads of 150 bases"""
    name = f"reads_hdist_best_batch_async seq+{off}"
    rng = rng_of(name)
    lens = [0, k - 1, k, 31, 32, 33] + [150] * 43
    offsets = rb.offsets_of(lens)
    n, count = int(offsets[-1]), len(lens)
    _, queries = _queries17(rng)
    return Spec(name, ab.bases(rng, n), off, scan_regions(n, off), [(4 * count, 0), (4 * count, 4), (count, 1)],
                lambda ctx, ptr, d, o: ctx.reads_hdist_best_batch_async(ptr, d["offsets"], count, n, k, d["queries"], Q17, *o),
                lambda oracle, s: list(rb.batch_best(s, offsets, k, queries)), {"offsets": offsets, "queries": queries})


# ---- per read, anchored ------------------------------------------------------------------------------------------------------------------
AK = 16
A_READ_LEN, A_COUNT = 151, 165  # an odd length: the read starts take all four byte alignments; two waves of 64 reads and 37 (clamped lanes)
A_SPANS = {"span19": (5, 8), "span64": (A_READ_LEN - AK - (ANCHOR_MAX_SPAN - AK), None)}  # pieces of 8 + 8 + 3; a 3' anchor of eight full pieces
GAP_READS = 4 * 256 + 4 * 25


def _anchored_cut(o, ln):
    """pieces of 8 bytes from the span's first byte: the first piece, the middle ones, the last (short where ln % 8)"""
    p, last = o // PIECE, (ln - 1) // PIECE
    return np.where(p == 0, 0, np.where(p == last, 2, 1))


def _edist_span_cut(o, ln):
    """the span's first four bytes, the middle, its last four (the dwords whose keep mask is partial at some alignment)"""
    return np.where(o < 4, 0, np.where(o >= ln - 4, 2, 1))


CUT_NAMES = {_anchored_cut: ("first piece", "middle pieces", "last piece"), _edist_span_cut: ("a span's first four bytes", "span middle", "a span's last four bytes")}


def span_layout(starts, lens, cut, full_reads):
    """spans [starts[r], starts[r] + lens[r]) (lens[r] == 0: none) -> (owned, regions): the spans of the reads below full_reads by `cut`, those of the
    last partial wave as a region of their own"""
    pos, reg = [], []
    for r, (a, ln) in enumerate(zip(starts, lens)):
        if ln:
            o = np.arange(int(ln))
            pos.append(int(a) + o)
            reg.append(cut(o, int(ln)) if r < full_reads else np.full(int(ln), 3))
    pos, reg = np.concatenate(pos), np.concatenate(reg)
    names = CUT_NAMES[cut] + ("the last partial wave (clamped lanes)",)
    return pos, [(names[i], pos[reg == i]) for i in range(4) if (reg == i).any()]


def _fixed_spans(read_len, count, k, lo, hi):
    hi_eff = read_len - k if hi is None else min(hi, read_len - k)
    span = hi_eff - lo + k
    assert 0 < span <= ANCHOR_MAX_SPAN
    return np.arange(count) * read_len + lo, np.full(count, span)


SIX = lambda count: [(4 * count, 0), (4 * count, 4), (count, 1), (4 * count, 8), (4 * count, 12), (count, 2)]  # noqa: E731


def reads_anchored(kind, which, count=A_COUNT, gaps=False):
    """kind: "hdist", "edist" or "pattern"; which: a key of A_SPANS"""
    lo, hi = A_SPANS[which]
    name = f"reads_{kind}_anchored_async {which} (pos_lo={lo} pos_hi={hi}) {A_READ_LEN} x {count}" + (" gaps" if gaps else "")
    rng = rng_of(name)
    n, off = A_READ_LEN * count, 7
    cut = _edist_span_cut if kind == "edist" else _anchored_cut
    owned, regions = span_layout(*_fixed_spans(A_READ_LEN, count, AK, lo, hi), cut, count // WAVE * WAVE)
    queries = ro.random_queries(rng, Q5, AK)
    good = ab.bases(rng, n)
    if kind == "hdist":
        call = lambda ctx, ptr, d, o: ctx.reads_hdist_anchored_async(ptr, A_READ_LEN, count, AK, d["queries"], Q5, *o, pos_lo=lo, pos_hi=hi)  # noqa: E731
        compute = lambda oracle, s: list(ra.reads_anchored(s, A_READ_LEN, count, AK, queries, lo, hi))  # noqa: E731
        inputs = {"queries": queries}
    elif kind == "edist":
        call = lambda ctx, ptr, d, o: ctx.reads_edist_anchored_async(ptr, A_READ_LEN, count, AK, d["queries"], Q5, *o, pos_lo=lo, pos_hi=hi)  # noqa: E731
        compute = lambda oracle, s: list(eo.reads_edist(s, A_READ_LEN, count, AK, queries, lo, hi))  # noqa: E731
        inputs = {"queries": queries}
    else:
        pats = np.stack([_pattern_with_n(int(q), AK, (2, 9)) for q in queries])
        call = lambda ctx, ptr, d, o: ctx.reads_pattern_anchored_async(ptr, A_READ_LEN, count, AK, d["patterns"], Q5, *o, pos_lo=lo, pos_hi=hi)  # noqa: E731
        compute = lambda oracle, s: list(rp.reads_anchored(s, A_READ_LEN, count, AK, pats, lo, hi))  # noqa: E731
        inputs = {"patterns": pats}
    spec = Spec(name, good, off, regions, SIX(count), call, compute, inputs, owned=owned)
    return gap_fill(spec) if gaps else spec


# the ragged batch: every length class of the header -- 0, 1 .. k - 1, k, k + pos_lo - 1 (no window), k + pos_lo, partial spans, full spans
A_RAGGED = {"start": ("start", 5, 8), "end": ("end", 0, ANCHOR_MAX_SPAN - AK)}  # START: spans of 16 .. 19 bases; END: 16 .. 64
A_LENS = tuple(rab.lengths_all_n(AK, 5, 4, extra=(40, 63, 64, 151, 33, 17, 19)))  # (an odd sum: every cycle starts at another byte lane)


def reads_anchored_batch(kind, which, cycles=6, gaps=False):
    anchor, lo, hi = A_RAGGED[which]
    name = f"reads_{kind}_anchored_batch_async {anchor.upper()} pos_lo={lo} pos_hi={hi}, {cycles} x {len(A_LENS)} reads" + (" gaps" if gaps else "")
    rng = rng_of(name)
    lens = list(A_LENS) * cycles
    offsets = rb.offsets_of(lens)
    n, count, off = int(offsets[-1]), len(lens), 3
    first, nwin = rab.windows(lens, AK, anchor, lo, hi)
    span = np.where(nwin > 0, nwin + AK - 1, 0)
    assert {0, AK - 1, AK + lo - 1, AK + lo} <= set(lens) and (span == hi - lo + AK).any() and ((span > 0) & (span < hi - lo + AK)).any()
    cut = _edist_span_cut if kind == "edist" else _anchored_cut
    owned, regions = span_layout(offsets[:-1].astype(np.int64) + first, span, cut, (count - 1) // WAVE * WAVE)
    queries = ro.random_queries(rng, Q5, AK)
    if kind == "hdist":
        call = lambda ctx, ptr, d, o: ctx.reads_hdist_anchored_batch_async(ptr, d["offsets"], count, n, AK, d["queries"], Q5, *o, pos_lo=lo, pos_hi=hi, anchor=anchor)  # noqa: E731
        compute = lambda oracle, s: list(rab.reads_anchored_batch(s, offsets, AK, queries, anchor, lo, hi))  # noqa: E731
    else:
        call = lambda ctx, ptr, d, o: ctx.reads_edist_anchored_batch_async(ptr, d["offsets"], count, n, AK, d["queries"], Q5, *o, pos_lo=lo, pos_hi=hi, anchor=anchor)  # noqa: E731
        compute = lambda oracle, s: list(eb.reads_edist_batch(s, offsets, AK, queries, anchor, lo, hi))  # noqa: E731
    spec = Spec(name, ab.bases(rng, n), off, regions, SIX(count), call, compute, {"offsets": offsets, "queries": queries}, owned=owned)
    return gap_fill(spec) if gaps else spec


# ---- per read, the whole read, edit distance --------------------------------------------------------------------------------------------------
E_READ_LEN, E_COUNT = 151, 293  # pieces of 64 + 64 + 23; one workgroup of 256 reads and 37


def _piece_cut(o, ln):
    p, last = o // EDIST_PIECE, (ln - 1) // EDIST_PIECE
    return np.where(p == 0, 0, np.where(p == last, 2, 1))


CUT_NAMES[_piece_cut] = ("first piece", "middle pieces", "last piece")


def reads_edist_best(kind):
    """kind: "edist" or "pattern" """
    name = f"reads_{'pattern_' if kind == 'pattern' else ''}edist_best_async {E_READ_LEN} x {E_COUNT}"
    rng = rng_of(name)
    n, off, count = E_READ_LEN * E_COUNT, 9, E_COUNT
    owned, regions = span_layout(np.arange(count) * E_READ_LEN, np.full(count, E_READ_LEN), _piece_cut, count // KC["kEdistBlock"] * KC["kEdistBlock"])
    queries = ro.random_queries(rng, Q5, EK)
    if kind == "edist":
        call = lambda ctx, ptr, d, o: ctx.reads_edist_best_async(ptr, E_READ_LEN, count, EK, d["queries"], Q5, *o)  # noqa: E731
        compute = lambda oracle, s: list(ebo.reads_edist_best(s, E_READ_LEN, count, EK, queries))  # noqa: E731
        inputs = {"queries": queries}
    else:
        pats = np.stack([_pattern_with_n(int(q), EK, (2, 9)) for q in queries])
        call = lambda ctx, ptr, d, o: ctx.reads_pattern_edist_best_async(ptr, E_READ_LEN, count, EK, d["patterns"], Q5, *o)  # noqa: E731
        compute = lambda oracle, s: list(ebo.reads_pattern_edist_best(s, E_READ_LEN, count, EK, pats))  # noqa: E731
        inputs = {"patterns": pats}
    return Spec(name, ab.bases(rng, n), off, regions, SIX(count), call, compute, inputs)


# inside one wave: lanes of unequal lengths and lanes that load nothing (the masked loop); the read of 63 bases (3 mod 4) stands in front of a read
# shorter than k, whose bytes are foreign
E_MIXED = (0, 63, EK - 1, EK, 64, 65, 128, 151, 200)


def reads_edist_best_batch(waves=1, gaps=False):
    """`waves` waves of mixed lengths, then a wave of 64 reads of 151 bases (the unmasked branch).  A read shorter than k is foreign."""
    name = f"reads_edist_best_batch_async {waves} mixed waves + an equal wave" + (" gaps" if gaps else "")
    rng = rng_of(name)
    mixed = [E_MIXED[i % len(E_MIXED)] for i in range(WAVE)]
    lens = (mixed + ([EK + 1] if gaps else [])) * waves + [E_READ_LEN] * WAVE  # (gaps: one more read makes a wave's sum odd -- every byte lane)
    offsets = rb.offsets_of(lens)
    n, count, off = int(offsets[-1]), len(lens), 6
    lens_a = np.asarray(lens)
    in_mixed = np.arange(count) < count - WAVE
    pos, reg = [], []
    for r in np.flatnonzero(lens_a >= EK):
        o = np.arange(lens_a[r])
        pos.append(int(offsets[r]) + o)
        reg.append(np.where(o < EDIST_PIECE, 0, 1) if in_mixed[r] else np.where(o < 2 * EDIST_PIECE, 2, 3))
    owned, reg = np.concatenate(pos), np.concatenate(reg)
    names = ("mixed wave, first pieces", "mixed wave, later pieces", "equal-length wave, whole pieces", "equal-length wave, last partial piece")
    regions = [(names[i], owned[reg == i]) for i in range(4)]
    queries = ro.random_queries(rng, Q5, EK)
    spec = Spec(name, ab.bases(rng, n), off, regions, SIX(count),
                lambda ctx, ptr, d, o: ctx.reads_edist_best_batch_async(ptr, d["offsets"], count, n, EK, d["queries"], Q5, *o),
                lambda oracle, s: list(ebo.reads_edist_best_batch(s, offsets, EK, queries)), {"offsets": offsets, "queries": queries}, owned=owned)
    return gap_fill(spec) if gaps else spec


# ---- every path: id -> (factory of the path's Spec, factory of its gap variant or None) --------------------------------------------------------
PATHS = {}
for _off in REF_OFFS:
    PATHS[f"kmer_hdist_best-ref+{_off}"] = (lambda o=_off: kmer_hdist_best(o), None)
    for _nb in (8, 16):
        PATHS[f"kmer_hdist_hist-{_nb}bins-ref+{_off}"] = (lambda o=_off, b=_nb: kmer_hdist_hist(o, b), None)
    for _cap in (False, True):
        PATHS[f"kmer_pattern_hits-{'capped' if _cap else 'cap0'}-ref+{_off}"] = (lambda o=_off, c=_cap: kmer_pattern_hits(o, c), None)
    PATHS[f"kmer_pattern_count_multi-ref+{_off}"] = (lambda o=_off: kmer_pattern_count_multi(o), None)
for _off in EDIST_REF_OFFS:
    PATHS[f"kmer_edist_best-ref+{_off}"] = (lambda o=_off: kmer_edist_best(o), None)
    PATHS[f"kmer_edist_count_multi-ref+{_off}"] = (lambda o=_off: kmer_edist_count_multi(o), None)
    for _above in (False, True):
        for _wd in (False, True):
            PATHS[f"kmer_edist_hits-cap-{'above' if _above else 'below'}-{'dist' if _wd else 'nodist'}-ref+{_off}"] = (
                lambda o=_off, a=_above, w=_wd: kmer_edist_hits(o, a, w), None)
PATHS["reads_hdist_best-150x44"] = (lambda: reads_hdist_best(150, 44, 6), None)
PATHS["reads_hdist_best-20x80"] = (lambda: reads_hdist_best(20, 80, 3, k=12), None)
PATHS["reads_hdist_best2-150x44"] = (lambda: reads_hdist_best(150, 44, 0, second=True), None)
PATHS["reads_hdist_best_batch"] = (lambda: reads_hdist_best_batch(), None)
for _kind in ("hdist", "edist"):
    for _which in A_SPANS:
        PATHS[f"reads_{_kind}_anchored-{_which}"] = (lambda k=_kind, w=_which: reads_anchored(k, w), lambda k=_kind, w=_which: reads_anchored(k, w, GAP_READS, True))
    for _which in A_RAGGED:
        PATHS[f"reads_{_kind}_anchored_batch-{_which}"] = (lambda k=_kind, w=_which: reads_anchored_batch(k, w),
                                                           lambda k=_kind, w=_which: reads_anchored_batch(k, w, 300, True))
PATHS["reads_pattern_anchored-span19"] = (lambda: reads_anchored("pattern", "span19"), lambda: reads_anchored("pattern", "span19", GAP_READS, True))
PATHS["reads_edist_best-151x293"] = (lambda: reads_edist_best("edist"), None)
PATHS["reads_edist_best_batch"] = (lambda: reads_edist_best_batch(), lambda: reads_edist_best_batch(160, True))
PATHS["reads_pattern_edist_best-151x293"] = (lambda: reads_edist_best("pattern"), None)
