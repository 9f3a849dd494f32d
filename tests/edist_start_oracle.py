"""The definition of bitnuc_reads_edist_start* / bitnuc_ref_edist_start*, as it stands in include/bitnuc_hip.h: for an item (text, floor a, query of k
positions, end e) with w = min(e - a, 2k - 1), the lexicographic minimum over s in [e - w, e] of (Lev(q, t[s, e)), e - s).  One full Levenshtein table PER
CANDIDATE SUBSTRING (lev: the scalar form; start_items: the same tables for all candidates of all items side by side in numpy) and the minimum over the
candidates -- no backward walk, no bit-parallel column, nothing of the product's or of the forward oracles' recurrence.
A query is k match masks: bit c of masks[i] set <=> base code c (A 0, C 1, G 2, T 3) matches position i."""
import numpy as np

FILL32 = 0xFFFFFFFF
FILL64 = 0xFFFFFFFFFFFFFFFF
W = 63  # 2 * 32 - 1: the widest window


def masks_of_query(q, k):
    """an exact 2-bit query: one singleton per position"""
    return np.array([1 << ((int(q) >> (2 * i)) & 3) for i in range(k)], dtype=np.uint8)


def masks_of_pattern(p, k):
    """a bitnuc_pattern (allow[c] bit i: code c matches position i)"""
    return np.array([sum(((int(p[c]) >> i) & 1) << c for c in range(4)) for i in range(k)], dtype=np.uint8)


def masks_of(queries, k):
    """(Q, k) masks of an array of exact queries (1-D) or of patterns ((Q, 4))"""
    q = np.asarray(queries)
    if q.ndim == 2:
        return np.stack([masks_of_pattern(p, k) for p in q]) if len(q) else np.zeros((0, k), dtype=np.uint8)
    return np.stack([masks_of_query(x, k) for x in q.reshape(-1)]) if q.size else np.zeros((0, k), dtype=np.uint8)


def lev(masks, codes):
    """the Levenshtein distance of the query to the whole string `codes`: the plain table, D[0][j] = j, D[i][0] = i"""
    n = len(codes)
    prev = list(range(n + 1))
    for i, m in enumerate(masks, 1):
        cur = [i] + [0] * n
        for j in range(1, n + 1):
            cur[j] = min(prev[j - 1] + (0 if (int(m) >> int(codes[j - 1])) & 1 else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[n]


def start_one(masks, codes, a, e):
    """(dist, start) of one item by the definition, one scalar table per candidate; codes: the whole text"""
    k = len(masks)
    w = min(e - a, 2 * k - 1)
    d, length = min((lev(masks, codes[s:e]), e - s) for s in range(e - w, e + 1))
    return d, e - length


def start_items(windows, ws, masks):
    """(dist, length) per item.  windows: (n, 63) codes, item r's w_r walked bases RIGHT-aligned (windows[r, 63 - w_r:] = t[e - w_r, e)); what is in front of
    them is never used.  ws: (n,) the w_r.  masks: (n, k).  Candidate c (0 <= c <= 63) of item r is the substring of its last c bases; every candidate has
    its own table (axis 1), filled row by row for all of them at once; the candidates with c > w_r are not candidates."""
    windows = np.asarray(windows, dtype=np.int64)
    ws = np.asarray(ws, dtype=np.int64)
    masks = np.asarray(masks, dtype=np.int64)
    n, k = masks.shape
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    c = np.arange(W + 1)[:, None]
    j = np.arange(1, W + 1)[None, :]
    idx = np.clip(W - c + j - 1, 0, W - 1)                  # candidate c's j-th base
    codes = np.where((j <= c)[None, :, :], windows[:, idx], 4)    # (n, 64, 63); 4: behind the candidate's last base, matches nothing
    cols = np.arange(W + 1)[None, None, :]
    prev = np.broadcast_to(cols, (n, W + 1, W + 1)).astype(np.int64)  # D[0][j] = j
    for i in range(1, k + 1):
        miss = 1 - ((masks[:, i - 1][:, None, None] >> codes) & 1)
        a = np.empty_like(prev)
        a[:, :, 0] = i
        a[:, :, 1:] = np.minimum(prev[:, :, :-1] + miss, prev[:, :, 1:] + 1)
        prev = np.minimum.accumulate(a - cols, axis=2) + cols      # cur[j] = min(a[j], cur[j - 1] + 1)
    cand = np.arange(W + 1)
    d = prev[:, cand, cand]                                        # candidate c's D[k][c]
    key = np.where(cand[None, :] <= ws[:, None], d * 64 + cand[None, :], 1 << 30)
    best = key.min(axis=1)
    return best >> 6, best & 63


def floor_of(length, k, anchor_end, pos):
    """the floor of a read: START: pos; END: len - k - pos, at least 0"""
    return max(0, length - k - pos) if anchor_end else pos


def starts(texts, floors, masks_q, k, query, end, fill=FILL32):
    """The outputs of a call: (start, dist) arrays.  texts[r]: the codes of item r's text (a sequence; one array for all items along a reference: pass
    [text] * n), floors[r] its floor, masks_q: (Q, k), query / end: per item.  Skipped items (query >= Q, end > len, end < floor; k == 0) get the fill."""
    n = len(end)
    start = np.full(n, fill, dtype=np.uint64)
    dist = np.full(n, 0xFF, dtype=np.uint8)
    live = [r for r in range(n) if k and int(query[r]) < len(masks_q) and floors[r] <= int(end[r]) <= len(texts[r])]
    if not live:
        return start, dist
    windows = np.zeros((len(live), W), dtype=np.int64)
    ws = np.zeros(len(live), dtype=np.int64)
    for i, r in enumerate(live):
        e = int(end[r])
        w = min(e - floors[r], 2 * k - 1)
        ws[i] = w
        if w:
            windows[i, W - w:] = np.asarray(texts[r][e - w:e], dtype=np.int64)
    d, length = start_items(windows, ws, masks_q[[int(query[r]) for r in live]])
    for i, r in enumerate(live):
        start[r] = int(end[r]) - int(length[i])
        dist[r] = int(d[i])
    return start, dist
