"""The definition of bitnuc_reads_edist_adapter* (include/bitnuc_hip.h) in numpy, never from the code under test: the plain DP over ALL rows, so that D[i][n]
is there for every prefix length i, each row's D[i][j-1] + 1 chain as a running minimum (the row form of reads_edist_best_oracle.long_read_columns, here
over every read and query of a batch at once), the candidates and their order as the header states them, and the cut as a direct Levenshtein minimum over
the admissible starts.

  allowed(i, num, den)                                     floor(i num / den)
  dp_rows(codes, k, patterns)                              (row_k, col_n): D[k][1..n] (R, Q, n) and D[0..k][n] (R, Q, k + 1) of R reads of n codes each
  lev(sets, codes)                                         the Levenshtein distance of a pattern prefix (a list of base sets, as 4-bit masks) to a text
  cut_of(sets, codes, e)                                   (dist, s): the lexicographic minimum over s in [e - min(e, 2i - 1), e] of (lev(sets, t[s:e]), e - s)
  reads_pattern_edist_adapter(s, read_len, count, k, patterns, min_overlap, num, den)      (adapter, cut, end, overlap, dist)
  reads_edist_adapter(s, read_len, count, k, queries, ...)                                 exact 2-bit queries
  reads_pattern_edist_adapter_batch(s, offsets, k, patterns, ...) / reads_edist_adapter_batch(s, offsets, k, queries, ...)   a ragged batch"""
import numpy as np

import reads_best_oracle as ro
import reads_pattern_oracle as rp

NO_U32 = 0xFFFFFFFF


def fill5(count):
    return (np.full(count, NO_U32, dtype=np.uint32), np.full(count, NO_U32, dtype=np.uint32), np.full(count, NO_U32, dtype=np.uint32),
            np.full(count, 0xFF, dtype=np.uint8), np.full(count, 0xFF, dtype=np.uint8))


def allowed(i, num, den):
    return (int(i) * int(num)) // int(den)


def dp_rows(codes, k, patterns):
    """codes: (R, n) base codes; patterns: (Q, 4) masks.  D[0][j] = 0, D[i][0] = i.  Row i from row i - 1: x[j] = min(D[i-1][j-1] + sub, D[i-1][j] + 1),
    x[0] = i, then D[i][j] = j + the running minimum of x[m] - m over m <= j."""
    t = np.asarray(codes, dtype=np.int64)
    nr, n = t.shape
    allow = rp.as_patterns(patterns).astype(np.int64)
    nq = allow.shape[0]
    ar = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros((nr, nq, n + 1), dtype=np.int64)
    col = np.zeros((nr, nq, k + 1), dtype=np.int64)
    for i in range(1, k + 1):
        bit = (allow >> (i - 1)) & 1                           # (Q, 4)
        sub = 1 - bit[np.arange(nq)[None, :, None], t[:, None, :]]  # (R, Q, n)
        x = np.empty_like(prev)
        x[:, :, 0] = i
        x[:, :, 1:] = np.minimum(prev[:, :, :-1] + sub, prev[:, :, 1:] + 1)
        prev = np.minimum.accumulate(x - ar, axis=2) + ar
        col[:, :, i] = prev[:, :, n]
    return prev[:, :, 1:], col


def sets_of(pattern, i):
    """the first i positions of one pattern ((4,) masks) as a list of 4-bit base sets"""
    p = [int(x) for x in np.asarray(pattern).reshape(4)]
    return [sum(((p[c] >> pos) & 1) << c for c in range(4)) for pos in range(i)]


def lev(sets, codes):
    """plain Levenshtein DP: sets[a] is the set (4-bit mask) of bases position a takes, codes the text"""
    codes = [int(c) for c in codes]
    prev = list(range(len(codes) + 1))
    for a, st in enumerate(sets, 1):
        cur = [a]
        for b, c in enumerate(codes, 1):
            cur.append(min(prev[b - 1] + (0 if (st >> c) & 1 else 1), prev[b] + 1, cur[b - 1] + 1))
        prev = cur
    return prev[-1]


def cut_of(sets, codes, e):
    """every start at once: Lev(a, b) = Lev(reversed a, reversed b), so the global DP of the reversed prefix against the reversed window has
    Lev(sets, t[e - c:e]) in its last row at column c"""
    i = len(sets)
    w = min(e, 2 * i - 1)
    back = np.asarray(codes[e - w:e], dtype=np.int64)[::-1]
    ar = np.arange(w + 1, dtype=np.int64)
    prev = ar.copy()
    for a in range(1, i + 1):
        st = sets[i - a]
        sub = 1 - ((st >> back) & 1)
        x = np.empty(w + 1, dtype=np.int64)
        x[0] = a
        x[1:] = np.minimum(prev[:-1] + sub, prev[1:] + 1)
        prev = np.minimum.accumulate(x - ar) + ar
    c = int(np.argmin(prev))  # the first minimum: the shortest substring
    return int(prev[c]), e - c


def _fixed_rows(codes, k, patterns, min_overlap, num, den, rows, out):
    """codes: (R, n) with n >= k: the results of these reads into out[...][rows]"""
    nr, n = codes.shape
    nq = patterns.shape[0]
    row_k, col = dp_rows(codes, k, patterns)
    full_d = row_k.min(axis=2)
    full_j = row_k.argmin(axis=2) + 1  # the first end that attains it
    # the candidates' order (misses, d, query, j) as one number per candidate, the smallest taken with numpy; none: NONE
    NONE = np.int64(1) << 62
    qs = np.arange(nq, dtype=np.int64)[None, :]

    keys = [np.where(full_d <= allowed(k, num, den), (full_d << 50) | (full_d << 44) | (qs << 27) | full_j, NONE)]
    which = [np.full((nr, nq), k, dtype=np.int64)]
    for i in range(min_overlap, k):
        d = col[:, :, i]
        keys.append(np.where(d <= allowed(i, num, den), ((k - i + d) << 50) | (d << 44) | (qs << 27) | n, NONE))
        which.append(np.full((nr, nq), i, dtype=np.int64))
    keys, which = np.concatenate(keys, axis=1), np.concatenate(which, axis=1)
    pick = keys.argmin(axis=1)
    for r in range(nr):
        key = int(keys[r, pick[r]])
        best = None if key == int(NONE) else (key >> 50, (key >> 44) & 63, (key >> 27) & 0x1FFFF, key & ((1 << 27) - 1), int(which[r, pick[r]]))
        if best is None:
            continue
        _, d, q, e, i = best
        dist, s = cut_of(sets_of(patterns[q], i), codes[r], e)
        assert dist == d, (dist, d)  # the definition's own consistency: the prefix's best substring ending at e has distance D[i][e]
        x = rows[r]
        out[0][x], out[1][x], out[2][x], out[3][x], out[4][x] = q, s, e, i, d


def reads_pattern_edist_adapter_batch(s, offsets, k, patterns, min_overlap, num, den):
    s = np.asarray(s, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    patterns = rp.as_patterns(patterns)
    count = off.size - 1
    out = [a.copy() for a in fill5(count)]
    if count == 0 or patterns.shape[0] == 0 or k == 0:
        return tuple(out)
    lens = np.diff(off)
    for m in np.unique(lens[lens >= k]):
        rows = np.nonzero(lens == m)[0]
        codes = ro.codes_of(s[(off[rows][:, None] + np.arange(int(m))[None, :]).reshape(-1)]).reshape(rows.size, int(m))
        uniq, back = np.unique(codes, axis=0, return_inverse=True)  # equal reads have equal answers: each is worked out once
        part = [a.copy() for a in fill5(uniq.shape[0])]
        _fixed_rows(uniq, k, patterns, min_overlap, num, den, np.arange(uniq.shape[0]), part)
        for a, b in zip(out, part):
            a[rows] = b[back.reshape(-1)]
    return tuple(out)


def reads_pattern_edist_adapter(s, read_len, count, k, patterns, min_overlap, num, den):
    return reads_pattern_edist_adapter_batch(np.asarray(s, dtype=np.uint8)[:count * read_len], np.arange(count + 1, dtype=np.uint64) * read_len, k, patterns,
                                             min_overlap, num, den)


def reads_edist_adapter_batch(s, offsets, k, queries, min_overlap, num, den):
    queries = np.asarray(queries, dtype=np.uint64).reshape(-1)
    if k == 0 or k > 32:
        return tuple(a.copy() for a in fill5(np.asarray(offsets).size - 1))
    return reads_pattern_edist_adapter_batch(s, offsets, k, rp.singletons(queries, k), min_overlap, num, den)


def reads_edist_adapter(s, read_len, count, k, queries, min_overlap, num, den):
    return reads_edist_adapter_batch(np.asarray(s, dtype=np.uint8)[:count * read_len], np.arange(count + 1, dtype=np.uint64) * read_len, k, queries,
                                     min_overlap, num, den)
