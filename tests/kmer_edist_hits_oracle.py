"""Expected values of the indel-tolerant hit list (bitnuc_kmer_edist_hits* and its bitnuc_kmer_pattern_edist_hits* twins), from kmer_edist_oracle.ends()
(the plain DP), never from the code under test: with e = E(1) .. E(n),  pos = nonzero(e <= tau) + 1  and  dist = e[pos - 1].

  hits(codes, k, pattern, tau)              (ends uint64 ascending, dists uint8), with the family's rule (k == 0 or n < k: nothing)
  sparse_hits(n, plants, k, pattern, tau)   the same on a reference of n bases that is all A except for `plants`, without a DP over all n columns"""
import numpy as np

import kmer_edist_oracle as ko


def of_ends(e, tau):
    at = np.nonzero(e <= int(tau))[0]
    return (at + 1).astype(np.uint64), e[at].astype(np.uint8)


def hits(codes, k, pattern, tau):
    if not ko.has_windows(len(codes), k):
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    return of_ends(ko.ends(codes, k, pattern), tau)


def sparse_hits(n, plants, k, pattern, tau):
    """kmer_edist_oracle.sparse_both's slicing: E(j) depends on the 2k bases before j only, so the DP on a slice that starts 2k bases early is exact from
    the slice's column 2k on, and the columns further than 2k behind every plant and behind the start share the background's value, which must exceed
    tau (the query is chosen that way): they hold no hit."""
    assert n >= 8 * k and all(0 <= p and p + len(c) <= n for p, c in plants)
    assert int(ko.ends(np.zeros(4 * k, dtype=np.int64), k, pattern)[-1]) > int(tau), "the background is a hit: not sparse"
    spans = sorted([(0, min(n, 4 * k))] + [(max(0, p - 2 * k), min(n, p + len(c) + 2 * k)) for p, c in plants])
    merged = [list(spans[0])]
    for lo, hi in spans[1:]:
        if lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    pos, dist = [], []
    for lo, hi in merged:  # columns lo .. hi - 1 (0-based): ends lo + 1 .. hi
        a = max(0, lo - 2 * k)
        text = np.zeros(hi - a, dtype=np.int64)
        for p, c in plants:
            s, t = max(p, a), min(p + len(c), hi)
            if s < t:
                text[s - a:t - a] = np.asarray(c)[s - p:t - p]
        e = ko.ends(text, k, pattern)[lo - a:]
        at = np.nonzero(e <= int(tau))[0]
        pos.append((at + lo + 1).astype(np.uint64))
        dist.append(e[at].astype(np.uint8))
    return np.concatenate(pos), np.concatenate(dist)
