"""Expected values of the anchored best match and runner-up per read (bitnuc_reads_hdist_anchored*), in numpy, never from the code under test: the
(count, read_len) matrix of the reads cut to the columns [pos_lo, hi_eff + k) -- hi_eff = min(pos_hi, read_len - k) --, reads_best2_oracle.reads_best2 on
that compact batch with read_len = span, and pos_lo added to both position arrays wherever they are not the fill.  No window (k == 0, read_len < k,
pos_lo > hi_eff, no queries): reads_best2_oracle.fill6.

  span_of(read_len, k, pos_lo, pos_hi)                               (hi_eff, span), or None without a window;  pos_hi None = to the end of the read
  reads_anchored(s, read_len, count, k, queries, pos_lo, pos_hi)     (query, pos, dist, second_query, second_pos, second_dist)
  compact(s, read_len, count, pos_lo, span)                          the spans as a batch of their own (bytes)"""
import numpy as np

import reads_best2_oracle as r2

NO_U32 = r2.NO_U32


def span_of(read_len, k, pos_lo=0, pos_hi=None):
    if k == 0 or read_len < k:
        return None
    hi = read_len - k if pos_hi is None else min(int(pos_hi), read_len - k)
    if pos_lo > hi:
        return None
    return hi, hi - pos_lo + k


def compact(s, read_len, count, pos_lo, span):
    m = np.asarray(s, dtype=np.uint8)[:count * read_len].reshape(count, read_len)
    return np.ascontiguousarray(m[:, pos_lo:pos_lo + span]).reshape(-1)


def reads_anchored(s, read_len, count, k, queries, pos_lo=0, pos_hi=None):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    hs = span_of(read_len, k, pos_lo, pos_hi)
    if hs is None or queries.size == 0 or count == 0:
        return r2.fill6(count)
    span = hs[1]
    out = r2.reads_best2(compact(s, read_len, count, pos_lo, span), span, count, k, queries)
    for pos in (out[1], out[4]):
        pos[pos != NO_U32] += np.uint32(pos_lo)
    return out
