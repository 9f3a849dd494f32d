"""Expected values of the indel-tolerant anchored match per read (bitnuc_reads_edist_anchored*, bitnuc_reads_pattern_edist_anchored*), in numpy from the
definition, never from the code under test: the plain dynamic programme, vectorised over the reads.

The span of read r is t_1 .. t_n = read_r[pos_lo .. hi_eff + k), hi_eff = min(pos_hi, read_len - k), n = hi_eff - pos_lo + k.  For a query of k positions
D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [t_j does not match position i], D[i-1][j] + 1, D[i][j-1] + 1); edist = min over 1 <= j <= n of
D[k][j], end = pos_lo + the smallest such j.  A query is a pattern, a (4,) uint32 array (pattern_oracle): allow[c] bit i set <=> base code c matches
position i; an exact query is its pattern of singletons.  The best is the lexicographic minimum of (edist, query, end), the runner-up the same minimum
over the OTHER queries (two equal queries are two queries); no span, and the runner-up with one query: the fill (2^32 - 1, 2^32 - 1, 255).

  span_of(read_len, k, pos_lo, pos_hi)                          n, or None without a span; pos_hi None = to the end of the read
  edist_columns(span_codes, k, patterns)                        (dist, j) per query and read: (Q, count) arrays, j in 1 .. n
  reads_edist(s, read_len, count, k, queries, pos_lo, pos_hi)   exact queries -> (query, end, dist, second_query, second_end, second_dist)
  reads_pattern_edist(s, ..., patterns, pos_lo, pos_hi)         patterns -> the same six
  plant(rng, query_codes, edits)                                a copy of a query with `edits` random edits, at least one of them an indel
  planted_cases()                                               five reads whose (dist, end) the tests assert by hand"""
import numpy as np

import reads_best_oracle as ro
import reads_pattern_oracle as rp

NO_U32 = rp.NO_U32
BIG = rp.BIG
fill6 = rp.fill6


def span_of(read_len, k, pos_lo=0, pos_hi=None):
    if k == 0 or read_len < k:
        return None
    hi = read_len - k if pos_hi is None else min(int(pos_hi), read_len - k)
    if pos_lo > hi:
        return None
    return hi - pos_lo + k


def edist_columns(t, k, patterns):
    """t: (count, n) codes, patterns: (Q, 4).  The DP row by row over the queries' positions, every row a (Q, count, n + 1) array -> (dist, j), (Q, count)
    each, j in 1 .. n the first column of the smallest D[k][j]."""
    t = np.asarray(t, dtype=np.int64)
    count, n = t.shape
    allow = rp.as_patterns(patterns).astype(np.int64)
    nq = allow.shape[0]
    prev = np.zeros((nq, count, n + 1), dtype=np.int32)  # D[0][j] = 0
    for i in range(1, k + 1):
        in_set = (allow >> (i - 1)) & 1                  # (Q, 4)
        sub = (1 - in_set[:, t]).astype(np.int32)        # (Q, count, n): [t_j does not match position i]
        cur = np.empty_like(prev)
        cur[:, :, 0] = i
        diag_or_up = np.minimum(prev[:, :, :-1] + sub, prev[:, :, 1:] + 1)
        for j in range(1, n + 1):                        # D[i][j-1] + 1 runs along the row
            cur[:, :, j] = np.minimum(diag_or_up[:, :, j - 1], cur[:, :, j - 1] + 1)
        prev = cur
    last = prev[:, :, 1:]
    j = last.argmin(axis=2)                              # the first of equal distances: the smallest end
    return np.take_along_axis(last, j[:, :, None], axis=2)[:, :, 0].astype(np.int64), j + 1


def reads_pattern_edist(s, read_len, count, k, patterns, pos_lo=0, pos_hi=None):
    patterns = rp.as_patterns(patterns)
    n = span_of(read_len, k, pos_lo, pos_hi)
    nq = patterns.shape[0]
    out = [a.copy() for a in fill6(count)]
    if n is None or nq == 0 or count == 0:
        return tuple(out)
    t = ro.codes_of(np.asarray(s, dtype=np.uint8)[:count * read_len]).reshape(count, read_len)[:, pos_lo:pos_lo + n]
    step = max(1, (1 << 22) // (count * (n + 1)))        # queries per slice: the DP rows stay small
    cols = [edist_columns(t, k, patterns[a:a + step]) for a in range(0, nq, step)]
    dmin = np.concatenate([c[0] for c in cols])          # (Q, count)
    jmin = np.concatenate([c[1] for c in cols])
    ar = np.arange(count)
    q1 = dmin.argmin(axis=0)                             # the first of equal distances: the smallest query
    out[0][:], out[1][:], out[2][:] = q1, jmin[q1, ar] + pos_lo, dmin[q1, ar]
    if nq > 1:
        rest = dmin.copy()
        rest[q1, ar] = BIG
        q2 = rest.argmin(axis=0)
        out[3][:], out[4][:], out[5][:] = q2, jmin[q2, ar] + pos_lo, rest[q2, ar]
    return tuple(out)


def reads_edist(s, read_len, count, k, queries, pos_lo=0, pos_hi=None):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    if span_of(read_len, k, pos_lo, pos_hi) is None:  # (k may be anything here: no pattern is made)
        return fill6(count)
    return reads_pattern_edist(s, read_len, count, k, rp.singletons(queries, k), pos_lo, pos_hi)


def plant(rng, codes, edits, indel=True):
    """codes with `edits` random edits (substitution to another base, insertion, deletion); indel: at least one is an insertion or a deletion"""
    out = [int(c) for c in codes]
    kinds = [int(rng.integers(0, 3)) for _ in range(edits)]
    if indel and edits and all(kd == 0 for kd in kinds):
        kinds[0] = int(rng.integers(1, 3))
    for kd in kinds:
        if kd == 0 and out:
            p = int(rng.integers(0, len(out)))
            out[p] = (out[p] + int(rng.integers(1, 4))) & 3
        elif kd == 1:
            out.insert(int(rng.integers(0, len(out) + 1)), int(rng.integers(0, 4)))
        elif len(out) > 1:
            del out[int(rng.integers(0, len(out)))]
    return np.array(out, dtype=np.int64)


def planted_cases():
    """one read per case, k = 16, the span [10, 40): a query with one deletion, one insertion, one substitution, two mixed edits, and an exact copy"""
    k, read_len, lo, n = 16, 60, 10, 30
    q = np.array([0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 1, 3])           # ACGTAACCGGTTAGCT
    other = np.array([3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2])       # TTTTTTTTTTTTTTTG: far from everything below
    bg = np.array([2, 2, 2, 2, 2, 2, 2, 2, 2, 2] * 6)                        # G background: q never aligns with it cheaply
    reads = []
    for variant in (np.delete(q, 5),                                         # one base of the AA run deleted: 15 bases
                    np.insert(q, 8, 3),                                      # a T inserted before position 8: 17 bases
                    np.where(np.arange(k) == 7, 0, q),                       # position 7 C -> A
                    np.insert(np.delete(q, 3), 9, 0),                        # position 3 deleted and an A inserted: 16 bases, two edits
                    q):
        c = bg.copy()
        c[lo + 4:lo + 4 + len(variant)] = variant
        reads.append(c)
    queries = np.array([ro.word_of(other), ro.word_of(q)], dtype=np.uint64)
    return k, read_len, lo, n, ro.LUT[np.concatenate(reads)].astype(np.uint8), queries
