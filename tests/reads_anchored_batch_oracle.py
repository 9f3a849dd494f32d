"""Expected values of the anchored best match and runner-up per read of a ragged batch (bitnuc_reads_hdist_anchored_batch*), in numpy, never from the
code under test.  Per read its admissible offsets are written down from the definition (windows), the reads are grouped by their NUMBER of admissible
offsets n, each group's spans (n + k - 1 bytes from the read's first admissible offset) are gathered into a compact fixed-length batch,
reads_best2_oracle.reads_best2 runs on it -- every admissible window against every query, top-2 over distinct queries, ties by the smallest query, then
the smallest offset -- and each read's first offset is added to both position arrays wherever they are not the fill.

  windows(lengths, k, anchor, pos_lo, pos_hi)                       (first, n) per read; anchor 0 / "start" or 1 / "end"; n == 0: no window
  reads_anchored_batch(s, offsets, k, queries, anchor, lo, hi)      (query, pos, dist, second_query, second_pos, second_dist)
  span_bytes(offsets, k, anchor, lo, hi)                            boolean mask over the batch's bytes: the bytes the call may read and validate
  lengths_all_n(k, pos_lo, offsets)                                 a mix of lengths with every number of admissible offsets"""
import numpy as np

import reads_best2_oracle as r2
import reads_batch_oracle as rb

NO_U32 = r2.NO_U32
START, END = 0, 1


def _end(anchor):
    return {"start": False, "end": True, 0: False, 1: True}[anchor]


def windows(lengths, k, anchor, pos_lo, pos_hi):
    """first admissible offset and number of admissible offsets per read, from the definition: START pos_lo <= i <= min(pos_hi, last); END
    pos_lo <= last - i <= pos_hi and i >= 0; last = len - k"""
    lengths = [int(x) for x in lengths]
    first = np.zeros(len(lengths), dtype=np.int64)
    n = np.zeros(len(lengths), dtype=np.int64)
    if k == 0 or pos_hi < pos_lo:
        return first, n
    for r, ln in enumerate(lengths):
        last = ln - k
        if last < 0:
            continue
        if _end(anchor):
            lo, hi = max(0, last - pos_hi), last - pos_lo
        else:
            lo, hi = pos_lo, min(pos_hi, last)
        if lo <= hi:
            first[r], n[r] = lo, hi - lo + 1
    return first, n


def reads_anchored_batch(s, offsets, k, queries, anchor="start", pos_lo=0, pos_hi=0):
    s = np.asarray(s, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    count = off.size - 1
    out = [a.copy() for a in r2.fill6(count)]
    if count == 0 or queries.size == 0:
        return tuple(out)
    first, n = windows(np.diff(off), k, anchor, pos_lo, pos_hi)
    for m in np.unique(n[n > 0]):
        rows = np.nonzero(n == m)[0]
        span = int(m) + k - 1
        at = off[rows] + first[rows]
        compact = s[(at[:, None] + np.arange(span)[None, :]).reshape(-1)]
        part = r2.reads_best2(compact, span, rows.size, k, queries)
        for i, a in enumerate(part):
            if i in (1, 4):
                a = np.where(a != NO_U32, a + first[rows].astype(np.uint32), a).astype(np.uint32)
            out[i][rows] = a
    return tuple(out)


def span_bytes(offsets, k, anchor, pos_lo, pos_hi):
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    first, n = windows(np.diff(off), k, anchor, pos_lo, pos_hi)
    mask = np.zeros(int(off[-1]), dtype=bool)
    for r in np.nonzero(n)[0]:
        mask[off[r] + first[r]:off[r] + first[r] + n[r] + k - 1] = True
    return mask


def lengths_all_n(k, pos_lo, offsets, extra=()):
    """lengths that give every number of admissible offsets 0 .. offsets (either anchor: n = min(len - k - pos_lo, offsets - 1) + 1), with 0, 1 .. k - 1, k,
    one base fewer than all offsets need, exactly enough, and much longer"""
    need = k + pos_lo
    ls = [0] + list(range(1, k)) + [k] + [need - 1 + j for j in range(offsets + 2) if need - 1 + j >= 0] + [need + offsets + 100, 300] + list(extra)
    return ls


pack_batch = rb.pack_batch
offsets_of = rb.offsets_of
word_offsets_of = rb.word_offsets_of
