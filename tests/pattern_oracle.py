"""Brute force of the pattern queries, straight from the definition: a pattern of length k is a set S_i of bases per position,
pdist(j) = #{ i < k : ref[j+i] not in S_i } for j in 0 .. n-k+1.  numpy only; nothing of the library is used here.  On top: the count, the first hits
with a cap, the leftmost arg-min.  A pattern is a (4,) uint32 array: allow[c] bit i set <=> base code c (A 0, C 1, G 2, T 3) is in S_i."""
import numpy as np

NO_POS = np.uint64(2**64 - 1)
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def codes_of_ascii(ref):
    """ASCII bases (either case) -> codes 0..3"""
    b = np.asarray(ref, dtype=np.uint8).astype(np.int64)
    return ((b >> 1) ^ (b >> 2)) & 3


def codes_of_words(words, n):
    """the first n bases of packed words -> codes 0..3"""
    w = np.asarray(words, dtype=np.uint64)
    i = np.arange(n)
    return ((w[i // 32] >> (2 * (i % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)


def pack_codes(codes, junk=0):
    """codes -> packed words; junk: bits ORed in above the last base"""
    n = len(codes)
    nw = (n + 31) // 32
    pad = np.zeros(nw * 32, dtype=np.uint64)
    pad[:n] = np.asarray(codes, dtype=np.uint64)
    words = np.bitwise_or.reduce(pad.reshape(nw, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1).astype(np.uint64) if nw else np.zeros(0, dtype=np.uint64)
    if n % 32:
        words[-1] |= np.uint64(junk & ~((1 << (2 * (n % 32))) - 1) & (2**64 - 1))
    return words


def from_sets(sets):
    """a list of k sets of codes -> pattern"""
    p = np.zeros(4, dtype=np.uint32)
    for i, s in enumerate(sets):
        for c in s:
            p[c] |= np.uint32(1 << i)
    return p


def from_iupac(letters):
    return from_sets([{CODE[b] for b in IUPAC[ch.upper()]} for ch in letters])


def from_2bit(query, k):
    return from_sets([{(int(query) >> (2 * i)) & 3} for i in range(k)])


def pdist(codes, pattern, k):
    """pdist of every window -> int64 array of max(n - k + 1, 0) entries (k == 0: none)"""
    codes = np.asarray(codes, dtype=np.intp)
    nwin = len(codes) - k + 1 if (k > 0 and len(codes) >= k) else 0
    d = np.zeros(nwin, dtype=np.uint8)  # at most k <= 32
    allow = [int(x) for x in np.asarray(pattern, dtype=np.uint32)]
    for i in range(k if nwin else 0):
        miss = np.array([1 - ((a >> i) & 1) for a in allow], dtype=np.uint8)  # [c not in S_i] for c = A, C, G, T
        d += miss.take(codes[i:i + nwin])
    return d.astype(np.int64)


def count(d, tau):
    return int((d <= tau).sum())


def hits(d, tau, cap):
    """(the first min(cap, total) positions, their distances, total)"""
    pos = np.flatnonzero(d <= tau)
    return pos[:cap].astype(np.uint64), d[pos[:cap]].astype(np.uint8), int(pos.size)


def best(d):
    """(leftmost arg-min, min); no windows: (2^64 - 1, 255)"""
    if d.size == 0:
        return NO_POS, np.uint8(0xFF)
    return np.uint64(int(np.argmin(d))), np.uint8(int(d.min()))


def random_sets(rng, k):
    """k random sets; about one position in eight is empty and one in eight is N"""
    out = []
    for _ in range(k):
        r = int(rng.integers(0, 8))
        out.append(set() if r == 0 else {0, 1, 2, 3} if r == 1 else {c for c in range(4) if rng.integers(0, 2)})
    return out
