"""Expected values of the per-read matchers under pattern queries (bitnuc_reads_pattern_best*, _best2*, _best_batch*, _anchored*, _anchored_batch*), in
numpy from the definitions, never from the code under test.  A pattern is a (4,) uint32 array (pattern_oracle): allow[c] bit i set <=> base code c is in
the set of position i; pdist of a window is pattern_oracle.pdist.  Per read and pattern the distances of the read's ADMISSIBLE windows are taken; the best
is the lexicographic minimum of (dist, query, offset), the runner-up the same minimum over the OTHER queries (two equal patterns are two queries; another
window of the winner never is the runner-up); a read without an admissible window, and the runner-up with one query: the fill (2^32 - 1, 2^32 - 1, 255).

  top2(codes, starts, first, n, k, patterns)                      the core: read r's windows are first[r] .. first[r] + n[r] - 1 from base starts[r]
  reads_best2(s, read_len, count, k, patterns)                    every window inside each read of a fixed-length batch -> six arrays
  reads_best_batch(s, offsets, k, patterns)                       ... of a ragged batch -> three arrays
  reads_anchored(s, read_len, count, k, patterns, lo, hi)         pos_lo <= i <= min(pos_hi, read_len - k) (pos_hi None: to the end) -> six arrays
  reads_anchored_batch(s, offsets, k, patterns, anchor, lo, hi)   START / END as the header defines them (reads_anchored_batch_oracle.windows) -> six"""
import numpy as np

import pattern_oracle as po
import reads_anchored_batch_oracle as rab

NO_U32 = np.uint32(0xFFFFFFFF)
NO_U8 = np.uint8(0xFF)
BIG = np.int64(1 << 20)  # above every distance


def fill6(count):
    return tuple(np.full(count, v, dtype=t) for v, t in ((NO_U32, np.uint32), (NO_U32, np.uint32), (NO_U8, np.uint8)) * 2)


def as_patterns(patterns):
    return np.ascontiguousarray(np.asarray(patterns, dtype=np.uint32).reshape(-1, 4))


def singletons(queries, k):
    return as_patterns([po.from_2bit(q, k) for q in np.asarray(queries, dtype=np.uint64).reshape(-1)]) if len(queries) else np.zeros((0, 4), dtype=np.uint32)


def top2(codes, starts, first, n, k, patterns):
    codes = np.asarray(codes, dtype=np.int64)
    starts, first, n = (np.asarray(a, dtype=np.int64) for a in (starts, first, n))
    patterns = as_patterns(patterns)
    count, nq = starts.size, patterns.shape[0]
    out = [a.copy() for a in fill6(count)]
    if count == 0 or nq == 0 or k == 0 or not (n > 0).any():
        return tuple(out)
    dist = np.stack([po.pdist(codes, p, k) for p in patterns])  # (Q, windows of the whole run): only windows inside a read are looked at
    for m in np.unique(n[n > 0]):
        rows = np.nonzero(n == m)[0]
        at = (starts[rows] + first[rows])[:, None] + np.arange(int(m))[None, :]
        d = dist[:, at]                                         # (Q, reads, offsets)
        omin = d.argmin(axis=2)                                 # the first of equal distances: the smallest offset
        dmin = np.take_along_axis(d, omin[:, :, None], axis=2)[:, :, 0]
        ar = np.arange(rows.size)
        q1 = dmin.argmin(axis=0)                                # the first of equal distances: the smallest query
        out[0][rows], out[1][rows], out[2][rows] = q1, omin[q1, ar] + first[rows], dmin[q1, ar]
        if nq > 1:
            rest = dmin.copy()
            rest[q1, ar] = BIG                                  # the winner is left out, every other query stays -- an equal pattern too
            q2 = rest.argmin(axis=0)
            out[3][rows], out[4][rows], out[5][rows] = q2, omin[q2, ar] + first[rows], rest[q2, ar]
    return tuple(out)


def reads_best2(s, read_len, count, k, patterns):
    codes = po.codes_of_ascii(np.asarray(s, dtype=np.uint8)[:count * read_len])
    nwin = read_len - k + 1 if 0 < k <= read_len else 0
    return top2(codes, np.arange(count) * read_len, np.zeros(count), np.full(count, nwin), k, patterns)


def reads_best_batch(s, offsets, k, patterns):
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    lens = np.diff(off)
    n = np.where(lens >= k, lens - k + 1, 0) if k > 0 else np.zeros_like(lens)
    return top2(po.codes_of_ascii(np.asarray(s, dtype=np.uint8)[:off[-1]]), off[:-1], np.zeros_like(lens), n, k, patterns)[:3]


def reads_anchored(s, read_len, count, k, patterns, pos_lo=0, pos_hi=None):
    last = read_len - k
    n = 0
    if k > 0 and last >= pos_lo:
        hi = last if pos_hi is None else min(pos_hi, last)
        n = max(hi - pos_lo + 1, 0)
    codes = po.codes_of_ascii(np.asarray(s, dtype=np.uint8)[:count * read_len])
    return top2(codes, np.arange(count) * read_len, np.full(count, pos_lo if n else 0), np.full(count, n), k, patterns)


def reads_anchored_batch(s, offsets, k, patterns, anchor="start", pos_lo=0, pos_hi=0):
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    first, n = rab.windows(np.diff(off), k, anchor, pos_lo, pos_hi)
    return top2(po.codes_of_ascii(np.asarray(s, dtype=np.uint8)[:off[-1]]), off[:-1], first, n, k, patterns)
