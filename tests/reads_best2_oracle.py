"""Expected values of the best match and the runner-up per read (bitnuc_reads_hdist_best2*), in numpy, never from the code under test: per query and
per read the minimum distance and its leftmost window; the best is the argmin over the queries (np.argmin returns the first minimum: the lowest query
wins a tie), the runner-up the argmin again with the winner's column masked out -- another window of the winning query is never the runner-up, and
an equal duplicate of the winning query at a higher index is.

  reads_best2(s, read_len, count, k, queries)            sliding_window_view over the (count, read_len) reshape, one query at a time
  reads_best2_by_scan(oracle, s, read_len, count, ...)   the oracle library's contiguous kmer_hdist_scan, inadmissible windows masked (the large cases)
  merge_top2(parts)                                      the top-2 over distinct queries of results on disjoint slices of the query list
All return (query, pos, dist, second_query, second_pos, second_dist) as np.uint32, np.uint32, np.uint8 twice; a read without a window, or no queries:
2^32 - 1, 2^32 - 1, 255 in all six; fewer than two queries: in the second triple."""
import numpy as np

import reads_best_oracle as ro

NO_U32 = ro.NO_U32
BIG = np.uint16(0x7FFF)  # above every distance: a masked column


def fill6(count):
    return ro.fill(count) + ro.fill(count)


def _top2(dmin, imin):
    """dmin, imin: (count, Q) per-query minimum distance and its leftmost window"""
    count, nq = dmin.shape
    rows = np.arange(count)
    out = fill6(count)
    b = np.argmin(dmin, axis=1)
    out[0][:], out[1][:], out[2][:] = b, imin[rows, b], dmin[rows, b]
    if nq >= 2:
        masked = dmin.astype(np.uint16)
        masked[rows, b] = BIG
        s = np.argmin(masked, axis=1)
        out[3][:], out[4][:], out[5][:] = s, imin[rows, s], dmin[rows, s]
    return out


def _per_query(rows_of, count, nq):
    dmin = np.empty((count, nq), dtype=np.uint8)
    imin = np.empty((count, nq), dtype=np.uint32)
    r = np.arange(count)
    for q in range(nq):
        d = rows_of(q)  # (count, windows)
        i = np.argmin(d, axis=1)
        dmin[:, q], imin[:, q] = d[r, i], i
    return dmin, imin


def reads_best2(s, read_len, count, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    if k == 0 or read_len < k or queries.size == 0 or count == 0:
        return fill6(count)
    c = ro.codes_of(np.asarray(s, dtype=np.uint8)[:count * read_len]).reshape(count, read_len)
    win = np.lib.stride_tricks.sliding_window_view(c, k, axis=1)  # (count, read_len - k + 1, k)
    return _top2(*_per_query(lambda q: (win != ro.query_codes(queries[q], k)).sum(axis=2).astype(np.uint8), count, queries.size))


def reads_best2_by_scan(oracle, s, read_len, count, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    if k == 0 or read_len < k or queries.size == 0 or count == 0:
        return fill6(count)
    s = np.ascontiguousarray(np.asarray(s, dtype=np.uint8)[:count * read_len])
    nw = read_len - k + 1

    def rows_of(q):
        d = np.full(count * read_len, 0xFF, dtype=np.uint8)
        scan = oracle.kmer_hdist_scan(s, k, int(queries[q]))
        d[:scan.size] = scan
        return d.reshape(count, read_len)[:, :nw]  # the windows that start in a read's last k - 1 bases cross into the next: masked
    return _top2(*_per_query(rows_of, count, queries.size))


def merge_top2(parts):
    """parts: [(first query index of the slice, six arrays of a call on that slice)], slices disjoint.  The candidates of a read are every slice's best
    and runner-up (distinct queries each); the overall best is their smallest (distance, query, offset), the runner-up the smallest of the others --
    exact, because a slice's third query is behind two others of its own slice."""
    count = parts[0][1][0].size
    keys = []
    for base, six in parts:
        for q, p, d in (six[:3], six[3:]):
            none = d == 0xFF
            key = (d.astype(np.uint64) << np.uint64(58)) | ((q.astype(np.uint64) + np.uint64(base)) << np.uint64(32)) | p.astype(np.uint64)
            key[none] = np.uint64(2**64 - 1)
            keys.append(key)
    keys = np.sort(np.stack(keys, axis=1), axis=1)[:, :2]  # distinct queries: distinct keys
    out = fill6(count)
    for j in range(2):
        key = keys[:, j]
        ok = key != np.uint64(2**64 - 1)
        out[3 * j][ok] = ((key[ok] >> np.uint64(32)) & np.uint64(0x3FFFFFF)).astype(np.uint32)
        out[3 * j + 1][ok] = (key[ok] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out[3 * j + 2][ok] = (key[ok] >> np.uint64(58)).astype(np.uint8)
    return out
