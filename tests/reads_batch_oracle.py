"""Expected values of the best match per read of a RAGGED batch (bitnuc_reads_hdist_best_batch*), in numpy, never from the code under test: read r is
s[offsets[r]:offsets[r + 1]]; for every read the lexicographically smallest (distance, query, offset) over all queries and the windows that lie
wholly inside the read.

  batch_best(s, offsets, k, queries)                 sliding_window_view per read, one read at a time (the small cases)
  batch_best_by_scan(scan, s, offsets, k, queries)   a contiguous scan of the concatenation per query -- scan(s, k, word) -> one distance per window:
                                                     the oracle library's kmer_hdist_scan, or numpy_scan below --, window j masked unless
                                                     j + k <= the end of its read, reduced per read (the large cases)
Both return (query, pos, dist) as np.uint32, np.uint32, np.uint8; a read without a window (empty, shorter than k), or no queries: 2^32 - 1,
2^32 - 1, 255.  pack_batch builds the words encode_batch writes, with junk (or chosen codes) in the pad bits."""
import numpy as np

import reads_best_oracle as ro

NO_U32 = ro.NO_U32
LUT = ro.LUT
fill = ro.fill
codes_of = ro.codes_of
query_codes = ro.query_codes
random_queries = ro.random_queries


def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def word_offsets_of(offsets):
    """the table encode_batch produces: ceil(len / 32) words per read"""
    off = np.asarray(offsets, dtype=np.uint64)
    return offsets_of((np.diff(off) + np.uint64(31)) // np.uint64(32))


def batch_best(s, offsets, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    off = [int(x) for x in np.asarray(offsets, dtype=np.uint64)]
    count = len(off) - 1
    query, pos, dist = fill(count)
    if k == 0 or queries.size == 0:
        return query, pos, dist
    c = codes_of(np.asarray(s, dtype=np.uint8))
    qc = np.stack([query_codes(w, k) for w in queries])  # (nq, k)
    for r in range(count):
        read = c[off[r]:off[r + 1]]
        if read.size < k:
            continue
        win = np.lib.stride_tricks.sliding_window_view(read, k)  # (windows, k)
        d = (win[None, :, :] != qc[:, None, :]).sum(axis=2)      # (nq, windows)
        m = d.min(axis=1)
        q = int(np.argmin(m))  # the first query with the smallest distance
        query[r], pos[r], dist[r] = q, int(np.argmin(d[q])), int(m[q])
    return query, pos, dist


def numpy_scan(s, k, word):
    """the contiguous distance scan in numpy: one distance per window of s"""
    c = codes_of(np.asarray(s, dtype=np.uint8))
    if c.size < k:
        return np.zeros(0, dtype=np.uint8)
    return (np.lib.stride_tricks.sliding_window_view(c, k) != query_codes(word, k)).sum(axis=1).astype(np.uint8)


def batch_best_by_scan(scan, s, offsets, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    off = np.asarray(offsets, dtype=np.int64)
    count = off.size - 1
    best = fill(count)
    n = int(off[-1])
    if k == 0 or queries.size == 0 or count == 0 or n < k:
        return best
    s = np.ascontiguousarray(np.asarray(s, dtype=np.uint8)[:n])
    j = np.arange(n, dtype=np.int64)
    read_of = np.searchsorted(off, j, side="right") - 1      # the last read that starts at or before j: never an empty one
    masked = j + k > off[read_of + 1]                          # the window crosses the end of its read
    live = np.nonzero(off[1:] > off[:-1])[0]                   # the reads that hold bases, in order: their starts cut the run
    starts = off[live]
    query, pos, dist = best
    for q, word in enumerate(queries):
        d = np.full(n, 0xFF, dtype=np.uint8)
        sc = scan(s, k, int(word))
        d[:sc.size] = sc
        d[masked] = 0xFF
        m = np.minimum.reduceat(d, starts)
        first = np.minimum.reduceat(np.where(d == np.repeat(m, np.diff(np.append(starts, n))), j, n), starts) - starts
        take = m < dist[live]  # ascending queries: a later one wins on a strictly smaller distance only (255 never wins)
        rows = live[take]
        query[rows], pos[rows], dist[rows] = q, first[take], m[take]
    return best


def pack_batch(s, offsets, junk=True, pad_codes=None, seed=0):
    """the words encode_batch writes for the ragged batch, the bits above a read's last base filled with junk, or with pad_codes[r] (a sequence of
    codes for read r's pad positions, shorter ones leave the rest junk) where given"""
    off = [int(x) for x in np.asarray(offsets, dtype=np.uint64)]
    count = len(off) - 1
    woff = word_offsets_of(offsets)
    total = int(woff[-1])
    if total == 0:
        return np.zeros(0, dtype=np.uint64)
    rng = np.random.default_rng(seed * 7919 + count)
    codes = rng.integers(0, 4, size=total * 32).astype(np.uint64) if junk else np.zeros(total * 32, dtype=np.uint64)
    c = codes_of(np.asarray(s, dtype=np.uint8)).astype(np.uint64)
    lens = np.diff(np.asarray(off, dtype=np.int64))
    dst0 = 32 * woff[:-1].astype(np.int64)
    idx = np.repeat(dst0 - np.asarray(off[:-1], dtype=np.int64), lens) + np.arange(off[-1], dtype=np.int64)  # base i of the batch -> its position in the words
    codes[idx] = c[:off[-1]]
    if pad_codes is not None:
        for r, pc in pad_codes.items():
            at = int(dst0[r]) + int(lens[r])
            room = 32 * int(woff[r + 1]) - at
            m = min(len(pc), room)
            codes[at:at + m] = np.asarray(pc[:m], dtype=np.uint64)
    w = np.bitwise_or.reduce(codes.reshape(total, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    return np.ascontiguousarray(w.astype(np.uint64))


def random_batch(rng, lengths, k, queries, plant=8, lower=0.3):
    """ASCII bases of a ragged batch, about 30 % lowercase, with mutated copies of the first queries planted inside reads that can hold them"""
    off = offsets_of(lengths)
    n = int(off[-1])
    codes = rng.integers(0, 4, size=n)
    lens = np.asarray(lengths, dtype=np.int64)
    can = np.nonzero(lens >= k)[0] if k else np.zeros(0, dtype=np.int64)
    if can.size:
        for i, q in enumerate(np.asarray(queries).reshape(-1)[:plant]):
            r = int(can[rng.integers(0, can.size)])
            p = int(off[r]) + int(rng.integers(0, lens[r] - k + 1))
            codes[p:p + k] = query_codes(q, k)
            if i % 2:
                codes[p + int(rng.integers(0, k))] = int(rng.integers(0, 4))
    s = LUT[codes].astype(np.uint8)
    s[rng.random(n) < lower] |= 0x20
    return s, off
