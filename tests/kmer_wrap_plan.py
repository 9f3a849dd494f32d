"""The case plan of tests/test_gpu_kmer_wrap.py: sizes at which the bounded grids of the sliding k-mer kernels wrap -- TEST INFRASTRUCTURE ONLY.

Every bounded-grid matrix-core kernel walks trips of U rounds of 1024 windows: wave w takes the trips w, w + nwaves, w + 2 nwaves, ... and, after its
first trip, loads the next one into the registers the current one has just left.  One PASS is nwaves * U rounds; below that size the trip loop runs
once.  plan(num_cu, k) mirrors the launchers' arithmetic (csrc/kmer.hip: bounded_grid) and returns, per kernel, sub-ranges (o, n) of ONE seeded
sequence -- window j's distance depends on s[j : j + k] only, so one oracle scan of the whole sequence gives the expected distances of every
sub-range -- whose round counts sit around one, two and three and a half passes, and, for the hit lists, whose per-trip counts fill just under,
exactly and just over one, two and three tiles of the two-level scan.

Pure Python + numpy: tests/test_kmer_wrap_plan.py checks the plan without a GPU (it re-derives every wave's trips) and compares the constants
below with the sources' text."""
from collections import namedtuple

import numpy as np

# ---- the launchers' constants (test_kmer_wrap_plan.py reads the same names out of the sources and compares)
K_BLOCK = 256         # device_prims.h: kBlock -- threads per workgroup of the single counts (four waves)
COUNT_ROUNDS = 4      # runtime.h: kCountRounds -- kmer_count3_mfma_kernel / packed_count3_mfma_kernel: rounds per trip
COUNT_GRID = 12       # runtime.h: kCountGrid -- ... workgroups per CU
MULTI_GRID = 1        # kmer.hip: kMultiGrid -- kmer_count3_multi_kernel / packed_count3_multi_kernel: workgroups per CU
MULTI_BLOCK = 768     # scan_multi_device.h: kMultiBlock -- ... threads per workgroup (twelve waves)
MULTI_ROUNDS = 4      # scan_multi_device.h: kMultiRounds -- ... rounds per trip
MULTI_QB = 16         # scan_multi_device.h: kMultiQB -- queries per grid.y block
HITS_TILE = 4096      # scan_hits_device.h: kHitsTile -- per-trip counts per tile of the hit lists' scan
HITS_ROUNDS = 4       # scan_hits_device.h: kHitsRounds -- rounds per trip (one workgroup of one wave each)
SCAN2_ROUNDS = 1      # kmer.hip: launch_count's count_scan2_t<false, false, 1, 0> -- the unaligned count: rounds per trip
SCAN2_WAVE_ROUNDS = 4 # kmer.hip: count_scan2_t's bounded_grid(.., (kBlock / 64) * 4, 8) -- rounds per WAVE that size its grid
SCAN2_GRID = 8        # ... workgroups per CU
ROUND = 1024          # windows per round; a round reads 1056 bases whatever k (scan_mfma_host.h: scan_rounds)

ASCII_OFFSETS = (0, 1, 7, 15)  # o mod 16: 0 -> the matrix-core single count; the others -> the bit-plane count, and skip = 16 - o mod 16 elsewhere
ANCHOR = 16                    # the dedicated cases (planted copies, invalid bytes) all start their rounds at absolute base ANCHOR: o + skip == ANCHOR

Kernel = namedtuple("Kernel", "name waves U per_wg per_cu packed")


def kernels():
    """name -> Kernel(waves per workgroup, rounds per trip, rounds per workgroup in bounded_grid's `want`, workgroups per CU)"""
    w, mw = K_BLOCK // 64, MULTI_BLOCK // 64
    return {
        "count3": Kernel("count3", w, COUNT_ROUNDS, w * COUNT_ROUNDS, COUNT_GRID, False),       # kmer.hip: count3_t
        "packed_count3": Kernel("packed_count3", w, 4, w * 4, COUNT_GRID, True),                 # kmer.hip: launch_count_packed
        "multi": Kernel("multi", mw, MULTI_ROUNDS, mw * MULTI_ROUNDS, MULTI_GRID, False),        # kmer.hip: multi_setup
        "packed_multi": Kernel("packed_multi", mw, 4, mw * MULTI_ROUNDS, MULTI_GRID, True),      # (a packed trip is four rounds)
        "scan2": Kernel("scan2", w, SCAN2_ROUNDS, w * SCAN2_WAVE_ROUNDS, SCAN2_GRID, False),      # kmer.hip: count_scan2_t
    }


def scan_rounds(n, skip=0):
    """scan_mfma_host.h: whole rounds in n bases whose first `skip` are left to the tail threads"""
    nr = n - skip if n > skip else 0
    return (nr - 32) >> 10 if nr >= 1056 else 0


def hits_trips(n, skip=0):
    """scan_hits_device.h"""
    return (scan_rounds(n, skip) + HITS_ROUNDS - 1) // HITS_ROUNDS


def bounded_grid(num_cu, rounds, per_wg, per_cu):
    """kmer.hip"""
    return min(rounds // per_wg + 1, num_cu * per_cu)


def ascii_skip(o):
    """the bases before the first 16-byte aligned one (kmer.hip: launch_hits, launch_count_multi), the buffer itself being 16-byte aligned"""
    return (16 - o % 16) % 16


def pass_rounds(kern, num_cu):
    """R: the rounds of one pass of the full grid"""
    return num_cu * kern.per_cu * kern.waves * kern.U


def round_targets(R):
    """The round counts of the sizes: around one pass (the first wave's second trip with every partial length), the same around two, and three
    and a half passes (a third full trip on half of the waves, a fourth, partial one behind them)."""
    return [R + d for d in range(-1, 6)] + [2 * R + d for d in range(-1, 6)] + [3 * R + R // 2 + 1]


def sizes_with_rounds(r, k, skip):
    """Four n with scan_rounds(n, skip) == r (r >= 1): the smallest (the fewest windows left to the tail threads), the one that leaves exactly
    k - 1 bases after the last window of the last round (the sequence's last window then starts on that window's last base), one in the middle
    and the largest (the most tail windows).  A round needs 32 bases beyond its 1024 whatever k, so for 2 k - 2 <= 32 the second size would
    have a round fewer: there the size with k - 1 bases beyond the last round's 1056 takes its place."""
    lo, hi = ROUND * r + 32, ROUND * r + 1055
    edge = ROUND * r + 2 * k - 2 if 2 * k - 2 > 32 else max(lo + k - 1, lo + 1)
    return [skip + lo, skip + edge, skip + lo + 517, skip + hi]


Case = namedtuple("Case", "kernel o n skip rounds tag")


def _case(kern, o, n, tag):
    if kern.packed:
        skip = 32 * ((o // 32) % 2)
    else:
        skip = 0 if kern.name in ("count3", "scan2") else ascii_skip(o)  # the single counts' rounds start at the pointer, aligned or not
    return Case(kern.name, o, n, skip, scan_rounds(n, skip), tag)


def plan(num_cu, k=31):
    """-> dict: P[kernel] (windows per pass), cases[kernel] (list of Case), length (bases of the sequence: about 3.6 of the largest pass),
    length_small (what the 12-wave kernels and the hit lists need), plants (absolute positions of exact copies of query 0), dedicated[family]
    ((rounds, bases) of the sub-range from ANCHOR on that the invalid-byte cases run on: three and a half passes)."""
    ks = kernels()
    P = {name: pass_rounds(kern, num_cu) * ROUND for name, kern in ks.items()}
    cases = {name: [] for name in ks}
    cases["hits"], cases["packed_hits"] = [], []
    # ASCII: the single counts' sizes come from the matrix-core count's pass; o mod 16 == 0 runs it, 1 / 7 / 15 the bit-plane count (whose
    # waves walk several one-round trips at any size, and whose grid is full at these sizes)
    for name in ("count3", "multi"):
        kern = ks[name]
        for ri, r in enumerate(round_targets(pass_rounds(kern, num_cu))):
            for oi, om in enumerate(ASCII_OFFSETS):
                skip = 0 if name == "count3" else ascii_skip(om)
                for vi, n in enumerate(sizes_with_rounds(r, k, skip)):
                    o = om + 16 * ((7 * ri + 3 * vi + oi) % 61)  # the sub-ranges start at different bases of the sequence
                    target = ks["scan2"] if (name == "count3" and om) else kern
                    c = _case(target, o, n, f"r{r}v{vi}")
                    assert c.rounds == r and c.skip == skip
                    assert bounded_grid(num_cu, r, target.per_wg, target.per_cu) == num_cu * target.per_cu  # the grid is full: a pass is R rounds
                    cases[target.name].append(c)
    for name in ("packed_count3", "packed_multi"):
        kern = ks[name]
        for ri, r in enumerate(round_targets(pass_rounds(kern, num_cu))):
            for wa in (0, 1):  # both word alignments: o / 32 even -> 16-byte aligned words, odd -> 8 mod 16 (skip = 32)
                for vi, n in enumerate(sizes_with_rounds(r, k, 32 * wa)):
                    o = 32 * (wa + 2 * ((5 * ri + 3 * vi) % 37))
                    c = _case(kern, o, n, f"r{r}v{vi}")
                    assert c.rounds == r and c.skip == 32 * wa
                    assert bounded_grid(num_cu, r, kern.per_wg, kern.per_cu) == num_cu * kern.per_cu
                    cases[name].append(c)
    # hit lists: hits_trips + 2 per-trip counts just below, at and just above one, two and three tiles; the last trip partial in three of four
    idx = 0
    for tiles in (1, 2, 3):
        for d in (-1, 0, 1):
            ntr = tiles * HITS_TILE + d
            for om in ASCII_OFFSETS + ("w0", "w1"):
                packed = isinstance(om, str)
                skip = (32 * int(om[1])) if packed else ascii_skip(om)
                r = HITS_ROUNDS * (ntr - 2) - idx % HITS_ROUNDS
                n = skip + ROUND * r + 32 + (131 * idx) % 1024
                o = 32 * (int(om[1]) + 2 * (idx % 29)) if packed else om + 16 * (idx % 53)
                c = Case("packed_hits" if packed else "hits", o, n, skip, r, f"tiles{tiles}{d:+d}")
                assert hits_trips(n, skip) + 2 == ntr and scan_rounds(n, skip) == r
                cases[c.kernel].append(c)
                idx += 1
    dedicated = dedicated_ranges(num_cu)
    need = lambda cs: max(c.o + c.n for c in cs)  # noqa: E731
    length_small = max(need(cases["multi"]), need(cases["packed_multi"]), need(cases["hits"]), need(cases["packed_hits"]),
                       ANCHOR + dedicated["multi"][1], ANCHOR + dedicated["hits"][1]) + 64
    length = max(need(cases["count3"]), need(cases["scan2"]), need(cases["packed_count3"]), ANCHOR + dedicated["count3"][1], length_small) + 64
    return {"P": P, "cases": cases, "length": length, "length_small": length_small, "dedicated": dedicated, "plants": plants(num_cu, k), "k": k}


def dedicated_ranges(num_cu):
    """family -> (rounds, bases): the sub-range from ANCHOR on that the planted-copy and invalid-byte cases run on -- three and a half passes and
    one round (a partial last trip); the hit lists: three tiles of per-trip counts, the last trip one round short"""
    ks, out = kernels(), {}
    for name in ("count3", "multi"):
        r = 3 * pass_rounds(ks[name], num_cu) + pass_rounds(ks[name], num_cu) // 2 + 1
        out[name] = (r, ROUND * r + 32 + 100)
    r = HITS_ROUNDS * (3 * HITS_TILE - 1) - 1
    out["hits"] = (r, ROUND * r + 32 + 100)
    return out


def tile_first_window(tile):
    """the first window (relative to the first round's) of the tile's first trip: per-trip count 0 is the head's, so tile t starts at trip
    t * kHitsTile - 1 (scan_hits_device.h: workgroup 1 + t takes trip t)"""
    return (tile * HITS_TILE - 1) * HITS_ROUNDS * ROUND


def plants(num_cu, k):
    """Absolute base positions at which an exact copy of query 0 is written over the background, for sub-ranges with o + skip == ANCHOR: per
    kernel family the last window of a pass, the first window of a pass, and a window that straddles the halo between two trips of different
    passes (each at a different pass boundary, so the copies do not overlap); either side of a tile boundary of the hit lists; window ANCHOR
    itself (the first window of a sub-range that starts there) and the last window of each dedicated sub-range.  Two plants are the same one or at least k bases apart."""
    ks = kernels()
    out = {ANCHOR: "first"}
    for i, name in enumerate(("count3", "multi", "scan2")):
        Pw = pass_rounds(ks[name], num_cu) * ROUND
        b = [(1, 2, 3), (2, 3, 1), (3, 1, 2)][i]
        out[ANCHOR + b[0] * Pw - 1] = f"{name}: last window of pass {b[0]}"
        out[ANCHOR + b[1] * Pw] = f"{name}: first window of pass {b[1] + 1}"
        out[ANCHOR + b[2] * Pw - max(k // 2, 1)] = f"{name}: across the halo into pass {b[2] + 1}"
    out[ANCHOR + tile_first_window(1) - 1] = "hits: last window before tile 1"
    out[ANCHOR + tile_first_window(2)] = "hits: first window of tile 2"
    for fam, (_, nb) in dedicated_ranges(num_cu).items():
        out[ANCHOR + nb - k] = f"{fam}: the last window of the dedicated sub-range"
    pos = sorted(out)
    for a, b in zip(pos, pos[1:]):
        assert b - a >= k, (a, b, out[a], out[b])
    return out


# ---- the data: a condition on the oracle's distances, not on random luck ---------------------------------------------------------------
def sensitive_taus(k):
    """the thresholds at which the generated data's per-window hit probability lies well inside (0, 1) (see make_sequence)"""
    return (0,) if k == 1 else (1, (3 * k) // 4)


def boundary_taus(k):
    return (0, 1, max(k - 1, 0), k, 2**32 - 1)


def make_query(k, seed):
    """-> (codes of the k bases, the packed query with junk above bit 2 k)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 4, size=k).astype(np.uint8)
    return q, query_word(q, int(rng.integers(1, 2**31)))


def query_word(q, junk):
    k = len(q)
    word = sum(int(c) << (2 * i) for i, c in enumerate(q))
    return (word | (junk << (2 * k))) & (2**64 - 1) if k < 32 else word


def rotate_query(q, by):
    """the query read from base `by` of its end-to-end repetition: in phase with the background at another residue"""
    r = np.roll(q, -by)
    return r, query_word(r, 0x5A5A5A5A + by)


def multi_queries(q):
    """At most six distinct queries for the multi-query counts, query 0 first: rotations of the query (each in phase with the background at
    another residue, so each has the same drifting hit probability); k = 1: the four bases."""
    k = len(q)
    if k == 1:
        return [((q + j) & 3, query_word((q + j) & 3, 0x1234567 + j)) for j in range(4)]
    rots = []
    for by in (0, 1, k // 2, k - 1, 5 % k, 3 % k):
        if by not in rots:
            rots.append(by)
    return [(q, query_word(q, 0x7654321))] + [rotate_query(q, by) for by in rots[1:]]


def make_sequence(length, q, seed, plants_at=()):
    """`length` ASCII bases, about 30 % lower case: the query repeated end to end, each base replaced by another one with a probability that
    drifts along the sequence: a seeded random level per 32768 bases in 0.01 .. 0.12, linear in between (k = 1: 0.10 .. 0.70, so that the share of
    the query's base drifts).  The drift has no period, so two trips a pass apart have unrelated hit probabilities whatever the pass length (a
    sine whose period divides the pass puts them in phase: 6.7 % equal trips at k = 16, tau = 1 on eight CUs).  Random bases alone leave most
    thresholds blind: at k = 31 hardly any window is within 0 or 8 of a random query, and a trip counted in place of another adds 0 - 0.
    Then exact copies of the query at plants_at."""
    k = len(q)
    lo, hi = (0.10, 0.70) if k == 1 else (0.01, 0.12)
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = np.empty(length, dtype=np.uint8)
    CH, BLK = 1 << 24, 1 << 15
    levels = lo + (hi - lo) * np.random.default_rng(seed ^ 0xD21F7).random(length // BLK + 2)
    for a in range(0, length, CH):
        m = min(CH, length - a)
        i = np.arange(a, a + m)
        f = ((i % BLK) / BLK).astype(np.float32)
        rate = levels[i // BLK].astype(np.float32) * (1 - f) + levels[i // BLK + 1].astype(np.float32) * f
        codes = q[i % k]
        mut = rng.random(m, dtype=np.float32) < rate
        codes = np.where(mut, (codes + rng.integers(1, 4, size=m, dtype=np.uint8)) & 3, codes)
        s[a:a + m] = lut[codes] | np.where(rng.integers(0, 256, size=m, dtype=np.uint8) < 77, 0x20, 0).astype(np.uint8)
    for j, p in enumerate(sorted(plants_at)):
        if p + k <= length:
            s[p:p + k] = lut[q] | (((np.arange(k) * 37 + j) & 1) * 0x20).astype(np.uint8)
    return s


def trip_hit_counts(dist, tau, first, trip_windows, ntrips):
    """the hits of ntrips consecutive trips of trip_windows windows from window `first` on (the oracle's distances)"""
    d = dist[first:first + trip_windows * ntrips]
    return (d <= min(tau, 255)).reshape(ntrips, trip_windows).sum(axis=1)


def sensitivity(dist, tau, first, trip_windows, ntrips, stride):
    """-> (share of the trips whose hit count equals that of the trip `stride` trips earlier -- the same wave's trip one pass earlier --,
    share of the trips with no hit or with every window a hit)"""
    c = trip_hit_counts(dist, tau, first, trip_windows, ntrips)
    same = float(np.mean(c[stride:] == c[:-stride])) if ntrips > stride else 1.0
    flat = float(np.mean((c == 0) | (c == trip_windows)))
    return same, flat


SENSITIVITY_CAP = 0.05  # at most 5 % of the trips may equal the trip one pass earlier, at most 5 % may have no hit or only hits


def check_sensitivity(dist, k, num_cu, first=ANCHOR, names=("count3", "multi", "scan2")):
    """The condition of the wrap tests, on the oracle's distances alone: for every sensitive threshold and every kernel, over the trips of the
    windows from `first` on.  -> the figures; raises AssertionError where a cap is missed."""
    ks, out = kernels(), {}
    for name in names:
        kern = ks[name]
        tw, stride = kern.U * ROUND, num_cu * kern.per_cu * kern.waves
        ntrips = (dist.size - first) // tw
        assert ntrips >= 2 * stride, (name, ntrips, stride)
        for tau in sensitive_taus(k):
            same, flat = sensitivity(dist, tau, first, tw, ntrips, stride)
            out[(name, tau)] = (same, flat)
            assert same <= SENSITIVITY_CAP and flat <= SENSITIVITY_CAP, (name, k, tau, same, flat)
    return out


def pack_words(s):
    """the packed words of an ASCII sequence (zero above 2 n in the last word)"""
    n = s.size
    nw = (n + 31) // 32
    codes = np.zeros(nw * 32, dtype=np.uint8)
    codes[:n] = ((s >> 1) ^ (s >> 2)) & 3
    c = codes.reshape(nw, 32)
    w = np.zeros(nw, dtype=np.uint64)
    for b in range(32):
        w |= c[:, b].astype(np.uint64) << np.uint64(2 * b)
    return w
