"""Expected values and reference data for the mismatch histogram per query (bitnuc_kmer_hdist_hist* / bitnuc_kmer_pattern_hist*).  Nothing of the
library is used here: the expected histogram is np.bincount over the oracle's distance scan (oracle_py.kmer_hdist_scan), for patterns over
pattern_oracle.pdist, truncated to n_bins.

Random k = 31 data leaves the bins 0 .. 15 empty and a test on zeros proves nothing, so `planted` builds a reference of random filler interleaved with
copies of the queries that carry m substitutions, m drawn uniformly from 0 .. n_bins (the first copy carries min(n_bins - 1, k): the last bin a window of
k bases can reach), and `assert_rich` states what every differential case holds its EXPECTED value to before the library is called: at least
ceil(b / 2) non-zero bins and a non-zero count in bin b - 1, where b = min(n_bins, k + 1) (a distance cannot exceed k, so the bins above k are empty by
definition).  The designated empty cases are those with fewer than 2 k n_bins windows (`roomy` is False): there is no room for the copies."""
import numpy as np

import pattern_oracle as po

LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def word(codes):
    return sum(int(c) << (2 * b) for b, c in enumerate(codes))


def codes_of_query(q, k):
    return np.array([(int(q) >> (2 * b)) & 3 for b in range(k)], dtype=np.int64)


def truncated(d, n_bins):
    """distances of every window -> the first n_bins bins of their histogram (uint64)"""
    return np.bincount(np.asarray(d, dtype=np.int64), minlength=n_bins)[:n_bins].astype(np.uint64)


def hist(oracle, s, k, queries, n_bins):
    """(n_queries, n_bins) uint64 by the oracle's scan of ASCII bases s; no windows: zeros"""
    out = np.zeros((len(queries), n_bins), dtype=np.uint64)
    if k == 0 or s.size < k:
        return out
    for i, q in enumerate(queries):
        out[i] = truncated(oracle.kmer_hdist_scan(s, k, int(q)), n_bins)
    return out


def pattern_hist(codes, patterns, k, n_bins):
    """(n_patterns, n_bins) uint64 by pattern_oracle.pdist over base codes"""
    out = np.zeros((len(patterns), n_bins), dtype=np.uint64)
    for i, p in enumerate(patterns):
        out[i] = truncated(po.pdist(codes, p, k), n_bins)
    return out


def roomy(n, k, n_bins):
    return k >= 1 and n - k + 1 >= 2 * k * n_bins


def substituted(rng, qc, m):
    """qc with exactly m positions changed to another base"""
    c = qc.copy()
    at = rng.choice(len(qc), size=m, replace=False)
    c[at] = (c[at] + rng.integers(1, 4, size=m)) & 3
    return c


def planted(rng, n, k, queries, n_bins, copies=64):
    """base codes of n bases: random filler, and in up to `copies` disjoint slots of 2 k bases a copy of a query (taken in turn) with m substitutions"""
    codes = rng.integers(0, 4, size=n)
    slots = n // (2 * k) if k else 0
    if slots == 0 or len(queries) == 0:
        return codes
    chosen = np.sort(rng.choice(slots, size=min(slots, copies), replace=False))
    for i, slot in enumerate(chosen):
        qc = codes_of_query(queries[i % len(queries)], k)
        m = min(n_bins - 1, k) if i == 0 else min(int(rng.integers(0, n_bins + 1)), k)
        p = int(slot) * 2 * k + int(rng.integers(0, k + 1))
        codes[p:p + k] = substituted(rng, qc, m)
    return codes


def ascii_of(rng, codes, lower=0.3):
    s = LUT[codes].astype(np.uint8)
    if lower:
        s[rng.random(s.size) < lower] |= 0x20
    return s


def assert_rich(h, k, n_bins):
    """on the EXPECTED histogram (all queries together), before the library is called"""
    b = min(n_bins, k + 1)
    total = np.asarray(h, dtype=np.uint64).reshape(-1, n_bins).sum(axis=0)
    assert int(np.count_nonzero(total[:b])) >= (b + 1) // 2 and int(total[b - 1]) > 0, (k, n_bins, total)
