"""Expected values of the indel-tolerant k-mer search along a reference (bitnuc_kmer_edist_best*, bitnuc_kmer_edist_count_multi* and their
bitnuc_kmer_pattern_edist_* twins), in numpy from the definition, never from the code under test.

The reference is t_1 .. t_n, a query has k positions.  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [t_j does not match position i],
D[i-1][j] + 1, D[i][j-1] + 1); E(j) = D[k][j], 1 <= j <= n.  best = (min_j E(j), the smallest j that attains it), count = #{ j : E(j) <= tau }.
The plain DP, row by row over the query's positions.  Inside a row the horizontal dependency cur[j] = min(x[j], cur[j-1] + 1), with
x[j] = min(diagonal, vertical) and x[0] = i, is a running minimum: cur[j] = min over l <= j of (x[l] + j - l) = minimum.accumulate(x - arange) + arange.
Every row is one numpy expression and nothing here is bit-parallel, so the oracle is independent of the kernel's and the host code's recurrence.
A query is a pattern, a (4,) uint32 array as in pattern_oracle (allow[c] bit i set <=> base code c matches position i); an exact query is its pattern
of singletons.

  ends(codes, k, pattern)            E(1) .. E(n) as an int64 array (n == 0: empty)
  best(e) / count(e, tau)            the two outputs from ends()' array; best of nothing: (2^64 - 1, 255)
  has_windows(n, k)                  the family's rule: k == 0 or n < k gives the fill and zeros although E(j) is defined
  kmer_edist_best(codes, k, patterns) / kmer_edist_count(codes, k, patterns, taus)   arrays over the queries, with that rule
  singletons(queries, k)             exact 2-bit queries -> (Q, 4) patterns"""
import numpy as np

import pattern_oracle as po

NO_END = po.NO_POS


def ends(codes, k, pattern):
    t = np.asarray(codes, dtype=np.intp)
    n = t.size
    allow = [int(x) for x in np.asarray(pattern, dtype=np.uint32)]
    ar = np.arange(n + 1, dtype=np.int32)
    prev = np.zeros(n + 1, dtype=np.int32)  # D[0][j] = 0
    for i in range(1, k + 1):
        miss = np.array([1 - ((a >> (i - 1)) & 1) for a in allow], dtype=np.int32)  # [c does not match position i] for c = A, C, G, T
        x = np.empty(n + 1, dtype=np.int32)
        x[0] = i
        np.minimum(prev[:-1] + miss.take(t), prev[1:] + 1, out=x[1:])
        prev = np.minimum.accumulate(x - ar) + ar
    return prev[1:].astype(np.int64)


def ends_three_term(codes, k, pattern):
    """the same by the three-term recurrence cell by cell: what ends() is checked against (slow)"""
    t = [int(c) for c in codes]
    allow = [int(x) for x in np.asarray(pattern, dtype=np.uint32)]
    prev = [0] * (len(t) + 1)
    for i in range(1, k + 1):
        cur = [i] * (len(t) + 1)
        for j in range(1, len(t) + 1):
            cur[j] = min(prev[j - 1] + (1 - ((allow[t[j - 1]] >> (i - 1)) & 1)), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return np.array(prev[1:], dtype=np.int64)


def best(e):
    if e.size == 0:
        return NO_END, np.uint8(0xFF)
    j = int(np.argmin(e))  # the first of equal distances: the smallest end
    return np.uint64(j + 1), np.uint8(int(e[j]))


def count(e, tau):
    return int((e <= int(tau)).sum())


def has_windows(n, k):
    return k > 0 and n >= k


def singletons(queries, k):
    q = np.asarray(queries, dtype=np.uint64).reshape(-1)
    return np.stack([po.from_2bit(int(x), k) for x in q]) if q.size else np.zeros((0, 4), dtype=np.uint32)


def as_patterns(patterns):
    return np.ascontiguousarray(np.asarray(patterns, dtype=np.uint32).reshape(-1, 4))


def kmer_edist_best(codes, k, patterns):
    p = as_patterns(patterns)
    end = np.full(p.shape[0], NO_END, dtype=np.uint64)
    dist = np.full(p.shape[0], 0xFF, dtype=np.uint8)
    if has_windows(len(codes), k):
        for q in range(p.shape[0]):
            end[q], dist[q] = best(ends(codes, k, p[q]))
    return end, dist


def kmer_edist_count(codes, k, patterns, taus):
    p = as_patterns(patterns)
    taus = np.broadcast_to(np.asarray(taus, dtype=np.int64), (p.shape[0],))
    out = np.zeros(p.shape[0], dtype=np.uint64)
    if has_windows(len(codes), k):
        for q in range(p.shape[0]):
            out[q] = count(ends(codes, k, p[q]), taus[q])
    return out


def sparse_both(n, plants, k, pattern, tau):
    """(end, dist, count) of one pattern on a reference of n bases that is all A except for `plants`, a list of (position, codes), without a DP over all
    n columns.  An optimal substring that ends at j has at most 2k bases (a longer one costs more than k, the empty one costs k), so E(j) depends on the
    2k bases before j only: the DP on a slice that starts 2k bases early is exact from the slice's column 2k on.  Columns further than 2k behind
    every plant and behind the start see A only and share one value, the background's; the others are computed slice by slice."""
    assert n >= 8 * k and all(0 <= p and p + len(c) <= n for p, c in plants)
    spans = sorted([(0, min(n, 4 * k))] + [(max(0, p - 2 * k), min(n, p + len(c) + 2 * k)) for p, c in plants])
    merged = [list(spans[0])]
    for lo, hi in spans[1:]:
        if lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    e_bg = int(ends(np.zeros(4 * k, dtype=np.int64), k, pattern)[-1])
    best_key, cnt, covered, first_bg = (1 << 62, 0), 0, 0, None
    at = 0
    for lo, hi in merged:  # columns lo .. hi - 1 (0-based): ends lo + 1 .. hi
        if first_bg is None and lo > at:
            first_bg = at
        at = hi
        a = max(0, lo - 2 * k)
        text = np.zeros(hi - a, dtype=np.int64)
        for p, c in plants:
            s, t = max(p, a), min(p + len(c), hi)
            if s < t:
                text[s - a:t - a] = np.asarray(c)[s - p:t - p]
        e = ends(text, k, pattern)[lo - a:]
        j = int(np.argmin(e))
        best_key = min(best_key, (int(e[j]), lo + j + 1))
        cnt += count(e, tau)
        covered += hi - lo
    if first_bg is None and at < n:
        first_bg = at
    if first_bg is not None:
        best_key = min(best_key, (e_bg, first_bg + 1))
        cnt += (n - covered) * (e_bg <= int(tau))
    return np.uint64(best_key[1]), np.uint8(best_key[0]), cnt


def kmer_edist_both(codes, k, patterns, taus):
    """(end, dist, counts) from one DP per query"""
    p = as_patterns(patterns)
    taus = np.broadcast_to(np.asarray(taus, dtype=np.int64), (p.shape[0],))
    end = np.full(p.shape[0], NO_END, dtype=np.uint64)
    dist = np.full(p.shape[0], 0xFF, dtype=np.uint8)
    cnt = np.zeros(p.shape[0], dtype=np.uint64)
    if has_windows(len(codes), k):
        for q in range(p.shape[0]):
            e = ends(codes, k, p[q])
            end[q], dist[q] = best(e)
            cnt[q] = count(e, taus[q])
    return end, dist, cnt
