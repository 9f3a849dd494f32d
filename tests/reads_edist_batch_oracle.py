"""Expected values of the indel-tolerant anchored match per read of a ragged batch (bitnuc_reads_edist_anchored_batch*, bitnuc_reads_pattern_edist_anchored_batch*),
in numpy, never from the code under test.  reads_anchored_batch_oracle.windows gives (first, n) per read from the definition of the admissible offsets; the
reads are grouped by n, each group's spans (n + k - 1 bytes from the read's first admissible offset) are gathered into a compact fixed-length batch,
reads_edist_oracle.reads_edist / reads_pattern_edist (the plain DP) runs on it over the whole span, and each read's `first` is added to both end arrays
wherever they are not the fill.

  reads_edist_batch(s, offsets, k, queries, anchor, lo, hi)             (query, end, dist, second_query, second_end, second_dist)
  reads_pattern_edist_batch(s, offsets, k, patterns, anchor, lo, hi)    the same for patterns ((Q, 4) uint32)"""
import numpy as np

import reads_anchored_batch_oracle as rab
import reads_edist_oracle as eo
import reads_pattern_oracle as rp

NO_U32 = eo.NO_U32
fill6 = eo.fill6
START, END = rab.START, rab.END


def reads_pattern_edist_batch(s, offsets, k, patterns, anchor="start", pos_lo=0, pos_hi=0):
    s = np.asarray(s, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    patterns = rp.as_patterns(patterns)
    count = off.size - 1
    out = [a.copy() for a in fill6(count)]
    if count == 0 or patterns.shape[0] == 0:
        return tuple(out)
    first, n = rab.windows(np.diff(off), k, anchor, pos_lo, pos_hi)
    for m in np.unique(n[n > 0]):
        rows = np.nonzero(n == m)[0]
        span = int(m) + k - 1
        at = off[rows] + first[rows]
        compact = s[(at[:, None] + np.arange(span)[None, :]).reshape(-1)]
        part = eo.reads_pattern_edist(compact, span, rows.size, k, patterns, 0, None)  # the whole compact read is the span
        for i, a in enumerate(part):
            if i in (1, 4):
                a = np.where(a != NO_U32, a + first[rows].astype(np.uint32), a).astype(np.uint32)
            out[i][rows] = a
    return tuple(out)


def reads_edist_batch(s, offsets, k, queries, anchor="start", pos_lo=0, pos_hi=0):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    count = np.asarray(offsets).size - 1
    if k == 0 or k > 32:  # no pattern is made
        return tuple(a.copy() for a in fill6(count))
    return reads_pattern_edist_batch(s, offsets, k, rp.singletons(queries, k), anchor, pos_lo, pos_hi)
