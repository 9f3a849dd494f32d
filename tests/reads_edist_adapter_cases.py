"""Planted reads for bitnuc_reads_edist_adapter*, with the five outputs worked out BY HAND from the definition in include/bitnuc_hip.h; shared by
tests/test_reads_edist_adapter_host.py (host forms) and tests/test_gpu_reads_edist_adapter.py (kernels, both layouts).  Every read has 30 bases; the insert is made
of C and T only and the adapters start with A, so no candidate arises by accident: an overhang of i positions needs the read's last i bases.

  CASES: (name, reads, adapters, min_overlap, num, den, want) with want a list of (adapter, cut, end, overlap, dist) per read, NONE for the fill."""
import numpy as np

K = 12
AD0 = "AGATCGGAAGAG"
AD1 = "AGATCGGTTTTT"  # shares AD0's first seven positions
BODY = "CTTCCTCTTCTCCTTCCTCTCTTCCTTCTC"
N = len(BODY)
NONE = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF, 0xFF)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def word_of(adapter):
    return sum(CODE[c] << (2 * i) for i, c in enumerate(adapter))


def ending(tail):
    """a read of N bases that ends with `tail`"""
    return BODY[:N - len(tail)] + tail


def sub(s, *at):
    """s with the bases at the given positions, none of them a C, replaced by C"""
    s = list(s)
    for i in at:
        assert s[i] != "C"
        s[i] = "C"
    return "".join(s)


CASES = [
    # allowed(i) = floor(i / 10): 0 below ten positions, 1 from ten on
    ("exact overhang of every length", [ending(AD0[:i]) for i in range(1, K)], [AD0], 1, 1, 10, [(0, N - i, N, i, 0) for i in range(1, K)]),
    # ten positions, one edit each: a substituted base, a base too many in the read, a base missing from the read
    ("overhang with one substitution", [ending(sub(AD0[:10], 5))], [AD0], 3, 1, 10, [(0, 20, 30, 10, 1)]),
    ("overhang with one insertion", [ending(AD0[:5] + "C" + AD0[5:10])], [AD0], 3, 1, 10, [(0, 19, 30, 10, 1)]),
    ("overhang with one deletion", [ending(AD0[:2] + AD0[3:10])], [AD0], 3, 1, 10, [(0, 21, 30, 10, 1)]),
    ("full adapter inside the read", [BODY[:10] + AD0 + BODY[:8]], [AD0], 3, 1, 10, [(0, 10, 22, 12, 0)]),
    # the read ends with eleven of twelve positions: the full candidate at j = n has (misses 1, d 1), the overhang of eleven (misses 1, d 0)
    ("full at the end against an equal-matches overhang", [ending(AD0[:11])], [AD0], 3, 1, 10, [(0, 19, 30, 11, 0)]),
    ("two adapters sharing a prefix", [ending(AD0[:7])], [AD0, AD1], 3, 1, 10, [(0, 23, 30, 7, 0)]),
    ("two adapters sharing a prefix, the other order", [ending(AD0[:7])], [AD1, AD0], 3, 1, 10, [(0, 23, 30, 7, 0)]),
    ("the second adapter's own tail decides", [ending(AD1[:9])], [AD0, AD1], 3, 1, 10, [(1, 21, 30, 9, 0)]),
    ("one base short of min_overlap", [ending(AD0[:4]), ending(AD0[:5])], [AD0], 5, 1, 10, [NONE, (0, 25, 30, 5, 0)]),
    # rate 1 / 5: ten positions allow two edits
    ("d = allowed and d = allowed + 1", [ending(sub(AD0[:10], 5, 8)), ending(sub(AD0[:10], 1, 5, 8))], [AD0], 8, 1, 5, [(0, 20, 30, 10, 2), NONE]),
    ("rate 0 / 1: exact only", [ending(AD0[:10]), ending(sub(AD0[:10], 5))], [AD0], 3, 0, 1, [(0, 20, 30, 10, 0), NONE]),
]


def random_reads(rng, lengths, k, nq, share=0.8):
    """(queries, ASCII bytes with lowercase among them, offsets): random reads of the given lengths; about `share` of the reads of at least k bases carry a
    prefix of a query -- of any length up to the whole query, half of them with one substitution, insertion or deletion -- at their END or, one in four,
    anywhere inside"""
    import reads_best_oracle as ro
    queries = rng.integers(0, 1 << 63, nq, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, nq, dtype=np.uint64)
    lengths = [int(x) for x in lengths]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    s = ro.LUT[rng.integers(0, 4, int(off[-1]))].astype(np.uint8)
    for r, n in enumerate(lengths):
        if n < k or rng.random() >= share:
            continue
        pre = [int(c) for c in ro.query_codes(queries[int(rng.integers(0, nq))], k)][:int(rng.integers(1, k + 1))]
        if len(pre) > 3 and rng.random() < 0.5:
            x, how = int(rng.integers(0, len(pre))), int(rng.integers(0, 3))
            if how == 0:
                pre[x] = (pre[x] + 1) % 4
            elif how == 1:
                pre.insert(x, int(rng.integers(0, 4)))
            else:
                del pre[x]
        pre = pre[:n]
        at = n - len(pre) if rng.random() < 0.75 else int(rng.integers(0, n - len(pre) + 1))
        s[int(off[r]) + at:int(off[r]) + at + len(pre)] = ro.LUT[np.asarray(pre, dtype=np.int64)]
    s = np.where(rng.random(s.size) < 0.3, s | 0x20, s).astype(np.uint8)
    return queries, s, off


def arrays(reads, adapters):
    """(ASCII bytes of the reads back to back, the adapters as 2-bit words)"""
    assert all(len(r) == N for r in reads)
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.array([word_of(a) for a in adapters], dtype=np.uint64)


def want_arrays(want):
    w = np.array(want, dtype=np.int64).reshape(-1, 5)
    return (w[:, 0].astype(np.uint32), w[:, 1].astype(np.uint32), w[:, 2].astype(np.uint32), w[:, 3].astype(np.uint8), w[:, 4].astype(np.uint8))
