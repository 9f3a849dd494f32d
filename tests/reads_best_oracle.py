"""Expected values of the best match per read (bitnuc_reads_hdist_best*), in numpy, never from the code under test: for every read of a fixed-length
batch the lexicographically smallest (distance, query, offset) over all queries and the windows that lie wholly inside the read.

  reads_best(s, read_len, count, k, queries)            sliding_window_view over the (count, read_len) reshape, one query at a time
  reads_best_by_scan(oracle, s, read_len, count, ...)   the oracle library's contiguous kmer_hdist_scan, inadmissible windows masked, reduced per read
                                                        (the large cases)
Both return (query, pos, dist) as np.uint32, np.uint32, np.uint8; a read without a window, or no queries: 2^32 - 1, 2^32 - 1, 255."""
import numpy as np

NO_U32 = np.uint32(2**32 - 1)
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def codes_of(s):
    """2-bit codes of ASCII bases, either case: A 0, C 1, G 2, T 3"""
    s = np.asarray(s, dtype=np.uint8)
    return ((s >> 1) ^ (s >> 2)) & 3


def query_codes(q, k):
    return np.array([(int(q) >> (2 * b)) & 3 for b in range(k)], dtype=np.uint8)


def word_of(codes):
    return sum(int(c) << (2 * b) for b, c in enumerate(codes))


def fill(count):
    return np.full(count, NO_U32, dtype=np.uint32), np.full(count, NO_U32, dtype=np.uint32), np.full(count, 0xFF, dtype=np.uint8)


def _merge(best, d, q):
    """fold query q's per-read distance rows d (count, windows) into best = (query, pos, dist): queries come in ascending order, so a later one wins on
    a strictly smaller distance only; argmin is the first minimum of a row"""
    query, pos, dist = best
    i = np.argmin(d, axis=1)
    m = d[np.arange(d.shape[0]), i]
    take = m < dist
    query[take], pos[take], dist[take] = q, i[take], m[take]


def reads_best(s, read_len, count, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    best = fill(count)
    if k == 0 or read_len < k or queries.size == 0 or count == 0:
        return best
    c = codes_of(np.asarray(s, dtype=np.uint8)[:count * read_len]).reshape(count, read_len)
    win = np.lib.stride_tricks.sliding_window_view(c, k, axis=1)  # (count, read_len - k + 1, k)
    for q, word in enumerate(queries):
        d = (win != query_codes(word, k)).sum(axis=2).astype(np.uint8)
        _merge(best, d, q)
    return best


def reads_best_by_scan(oracle, s, read_len, count, k, queries):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    best = fill(count)
    if k == 0 or read_len < k or queries.size == 0 or count == 0:
        return best
    s = np.ascontiguousarray(np.asarray(s, dtype=np.uint8)[:count * read_len])
    nw = read_len - k + 1
    for q, word in enumerate(queries):
        d = np.full(count * read_len, 0xFF, dtype=np.uint8)
        scan = oracle.kmer_hdist_scan(s, k, int(word))
        d[:scan.size] = scan
        _merge(best, d.reshape(count, read_len)[:, :nw], q)  # the windows that start in a read's last k - 1 bases cross into the next: masked
    return best


def pack_reads(s, read_len, count, junk=True, pad_codes=None):
    """the words encode_fixed writes for back-to-back reads, the bits above 2 * read_len of a read's last word filled with junk, or with pad_codes
    (count, 32 * wpr - read_len)"""
    wpr = (read_len + 31) // 32
    if count == 0 or wpr == 0:
        return np.zeros(0, dtype=np.uint64)
    pad = np.zeros((count, wpr * 32), dtype=np.uint64)
    pad[:, :read_len] = codes_of(np.asarray(s, dtype=np.uint8)[:count * read_len]).reshape(count, read_len)
    if pad_codes is not None:
        pad[:, read_len:] = pad_codes
    elif junk and read_len % 32:
        pad[:, read_len:] = np.random.default_rng(read_len * 7919 + count).integers(0, 4, size=(count, wpr * 32 - read_len))
    w = np.bitwise_or.reduce(pad.reshape(count * wpr, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    return np.ascontiguousarray(w.astype(np.uint64))


def random_queries(rng, nq, k):
    """random queries with junk above 2k"""
    return rng.integers(0, 2**63, size=nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=nq, dtype=np.uint64)


def random_reads(rng, read_len, count, k, queries, plant=8, lower=0.3):
    """count * read_len ASCII bases, about 30 % lowercase, with mutated copies of the first queries planted inside reads"""
    n = read_len * count
    codes = rng.integers(0, 4, size=n)
    if read_len >= k and k and count:
        for i, q in enumerate(np.asarray(queries).reshape(-1)[:plant]):
            r, p = int(rng.integers(0, count)), int(rng.integers(0, read_len - k + 1))
            codes[r * read_len + p:r * read_len + p + k] = query_codes(q, k)
            if i % 2:
                codes[r * read_len + p + int(rng.integers(0, k))] = int(rng.integers(0, 4))
    s = LUT[codes].astype(np.uint8)
    s[rng.random(n) < lower] |= 0x20
    return s
