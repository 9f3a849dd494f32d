"""Expected values of the indel-tolerant best match per read over the WHOLE read (bitnuc_reads_edist_best*, _best_batch* and their pattern twins), in numpy,
never from the code under test: reads_edist_oracle.reads_edist / reads_pattern_edist (the plain DP) with pos_lo = 0, pos_hi = None -- the whole read is the
span; it takes any read length.  A ragged batch is grouped by length: the reads of one length are gathered into a compact fixed-length batch, the DP runs
on it, and the results go back to their rows; a read shorter than k keeps the fill.

  reads_edist_best(s, read_len, count, k, queries)            (query, end, dist, second_query, second_end, second_dist)
  reads_pattern_edist_best(s, read_len, count, k, patterns)   the same for patterns ((Q, 4) uint32)
  reads_edist_best_batch(s, offsets, k, queries)              a ragged batch
  reads_pattern_edist_best_batch(s, offsets, k, patterns)
  long_read_columns(codes, k, patterns)                       (dist, j) per query for ONE long read: the same DP, each row's D[i][j-1] + 1 chain as a
                                                              running minimum (np.minimum.accumulate) instead of a Python loop over j
  hamming_best_dist(s, offsets, k, queries)                   per read the smallest Hamming distance over queries and windows (255 without a window)"""
import numpy as np

import reads_best_oracle as ro
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

NO_U32 = eo.NO_U32
fill6 = eo.fill6


def reads_pattern_edist_best(s, read_len, count, k, patterns):
    return eo.reads_pattern_edist(s, read_len, count, k, patterns, 0, None)


def reads_edist_best(s, read_len, count, k, queries):
    if k == 0 or k > 32:  # no pattern is made
        return tuple(a.copy() for a in fill6(count))
    return eo.reads_edist(s, read_len, count, k, queries, 0, None)


def reads_pattern_edist_best_batch(s, offsets, k, patterns):
    s = np.asarray(s, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    patterns = rp.as_patterns(patterns)
    count = off.size - 1
    out = [a.copy() for a in fill6(count)]
    if count == 0 or patterns.shape[0] == 0 or k == 0:
        return tuple(out)
    lens = np.diff(off)
    for m in np.unique(lens[lens >= k]):
        rows = np.nonzero(lens == m)[0]
        compact = s[(off[rows][:, None] + np.arange(int(m))[None, :]).reshape(-1)]
        part = eo.reads_pattern_edist(compact, int(m), rows.size, k, patterns, 0, None)
        for i, a in enumerate(part):
            out[i][rows] = a
    return tuple(out)


def reads_edist_best_batch(s, offsets, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    count = np.asarray(offsets).size - 1
    if k == 0 or k > 32:
        return tuple(a.copy() for a in fill6(count))
    return reads_pattern_edist_best_batch(s, offsets, k, rp.singletons(queries, k))


def long_read_columns(codes, k, patterns):
    """One read of n codes against Q patterns -> (dist, j), (Q,) each.  Row i of the DP from row i - 1: x[j] = min(D[i-1][j-1] + sub, D[i-1][j] + 1), x[0] = i,
    then D[i][j] = min over m <= j of x[m] + (j - m) = j + the running minimum of x[m] - m."""
    t = np.asarray(codes, dtype=np.int64)
    n = t.size
    allow = rp.as_patterns(patterns).astype(np.int64)
    nq = allow.shape[0]
    ar = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros((nq, n + 1), dtype=np.int64)
    for i in range(1, k + 1):
        sub = 1 - ((allow >> (i - 1)) & 1)[:, t]
        x = np.empty_like(prev)
        x[:, 0] = i
        x[:, 1:] = np.minimum(prev[:, :-1] + sub, prev[:, 1:] + 1)
        prev = np.minimum.accumulate(x - ar, axis=1) + ar
    last = prev[:, 1:]
    j = last.argmin(axis=1)
    return last[np.arange(nq), j], j + 1


def six_of_columns(dist, j):
    """the six outputs of ONE read from its per-query (dist, j)"""
    out = [a.copy() for a in fill6(1)]
    q1 = int(np.argmin(dist))
    out[0][0], out[1][0], out[2][0] = q1, j[q1], dist[q1]
    if dist.size > 1:
        rest = dist.copy()
        rest[q1] = 1 << 30
        q2 = int(np.argmin(rest))
        out[3][0], out[4][0], out[5][0] = q2, j[q2], rest[q2]
    return tuple(out)


def hamming_best_dist(s, offsets, k, queries):
    s = np.asarray(s, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    qc = np.stack([ro.query_codes(q, k) for q in np.asarray(queries, dtype=np.uint64).reshape(-1)])  # (Q, k)
    out = np.full(off.size - 1, 255, dtype=np.int64)
    for r in range(off.size - 1):
        c = ro.codes_of(s[off[r]:off[r + 1]]).astype(np.int64)
        if c.size < k:
            continue
        win = np.lib.stride_tricks.sliding_window_view(c, k)  # (W, k)
        out[r] = (win[None, :, :] != qc[:, None, :]).sum(axis=2).min()
    return out
