"""All 256 byte values in and beside the ASCII input of the three ASCII paths of edist_start_kernel (-m gpu): bitnuc_reads_edist_start_async (fixed),
bitnuc_reads_edist_start_batch_async (ragged) and bitnuc_ref_edist_start_async (along a reference), in the manner of tests/test_gpu_alphabet_search.py
with tests/alphabet.py's classes and reject_plan.

OWNED positions are the walked ranges as the header block states them: of a live item the w = min(e - a, 2k - 1) bytes in front of its end, nothing else
-- not the rest of its read, not a byte of a skipped item's read, not the bytes around the buffer.
ACCEPT: upper, lower and mixed case give the oracle's result.  REJECT: each of the 248 invalid values once at each byte lane of a dword (992 cases per
path, rotating over the path's regions: a window's first bytes, its interior, its last bytes); the error is the first invalid OWNED byte in buffer order
-- a later one of the other class never wins --, the next sync is clean, and a clean call follows the sweep.  IGNORE: every byte that is not owned takes
each of the 256 values: the call succeeds with the oracle's result."""
import numpy as np
import pytest

import alphabet as al
import edist_start_oracle as so
import reads_batch_oracle as rb
import reads_best_oracle as ro

pytestmark = pytest.mark.gpu

K = 16
PAD = 64  # bytes around the input in its device buffer: not owned


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


class StartPath:
    """one ASCII path: the clean input, its items, the walked range of every live item and the call on a device buffer"""

    def __init__(self, ctx, kind):
        import torch
        rng = np.random.default_rng({"fixed": 11, "ragged": 12, "reference": 13}[kind])
        self.ctx, self.kind, self.torch = ctx, kind, torch
        self.queries = ro.random_queries(rng, 3, K)
        self.dq = _dev(self.queries)
        if kind == "reference":
            n, m = 40_000, 333
            self.lens = [n]
            self.off = np.array([0, n], dtype=np.uint64)
            self.end = np.sort(rng.choice(np.arange(40, n - 40, 97), size=m, replace=False)).astype(np.uint64)  # windows apart: bytes between them are foreign
            self.end[:8] = [0, 1, 2, 3, 30, 31, 32, 33]
            self.end[-2:] = [n, n + 1]
            self.query = rng.integers(0, 4, size=m).astype(np.uint32)  # 3: no such query
            self.floors = [0] * m
            self.text_of = [0] * m
            self.wide = True
        else:
            count = 333
            lens = np.full(count, 100) if kind == "fixed" else rng.integers(0, 201, size=count)
            self.lens = [int(x) for x in lens]
            self.off = rb.offsets_of(lens)
            self.anchor, self.pos = (0, 5) if kind == "fixed" else (1, 3)
            self.floors = [so.floor_of(ln, K, self.anchor, self.pos) for ln in self.lens]
            self.end = np.array([max(0, int(rng.integers(f - 1, max(ln, f) + 2))) for f, ln in zip(self.floors, self.lens)], dtype=np.uint32)
            self.end[:64] = [min(ln, 60) for ln in self.lens[:64]]
            self.query = rng.integers(0, 4, size=count).astype(np.uint32)
            self.text_of = list(range(count))
            self.wide = False
        total = int(self.off[-1])
        self.good = al.bases(rng, total, "upper")
        # the walked ranges, in buffer coordinates
        owned = np.zeros(total, dtype=bool)
        first, inner, last = [], [], []
        for i, (e, q) in enumerate(zip(self.end, self.query)):
            t = self.text_of[i]
            e, a, ln = int(e), self.floors[i], self.lens[t]
            if q >= 3 or e > ln or e < a:
                continue
            w = min(e - a, 2 * K - 1)
            lo = int(self.off[t]) + e - w
            owned[lo:lo + w] = True
            first += list(range(lo, lo + min(w, 4)))
            last += list(range(lo + max(0, w - 4), lo + w))
            inner += list(range(lo + 4, lo + w - 4))
        self.owned = owned
        self.regions = [("a window's first bytes", first), ("a window's interior", inner), ("a window's last bytes", last)]
        self.buf = torch.zeros(total + 2 * PAD, dtype=torch.uint8, device="cuda:0")
        self.d_off = _dev(self.off)
        self.d_query, self.d_end = _dev(self.query), _dev(self.end)
        n_items = len(self.end)
        self.start = torch.zeros(n_items, dtype=torch.int64 if self.wide else torch.int32, device="cuda:0")
        self.dist = torch.zeros(n_items, dtype=torch.uint8, device="cuda:0")

    def want(self, s):
        codes = ro.codes_of(s)
        texts = [codes[int(self.off[t]):int(self.off[t + 1])] for t in range(len(self.off) - 1)]
        ws, wd = so.starts([texts[t] for t in self.text_of], self.floors, so.masks_of(self.queries, K), K, self.query, self.end,
                           fill=so.FILL64 if self.wide else so.FILL32)
        return ws, wd

    def run(self, s, around=0):
        """the call on the bytes s (the bytes around them: `around`) -> (start, dist) after a sync, which raises the call's error"""
        torch, c = self.torch, self.ctx
        self.buf.fill_(around)
        self.buf[PAD:PAD + s.size] = torch.from_numpy(s)
        self.start.fill_(0x5A), self.dist.fill_(0x5A)
        ptr = self.buf.data_ptr() + PAD
        n_items = len(self.end)
        if self.kind == "fixed":
            c.reads_edist_start_async(ptr, 100, n_items, K, self.dq, 3, self.d_query, self.d_end, self.start, self.dist, "start", self.pos)
        elif self.kind == "ragged":
            c.reads_edist_start_batch_async(ptr, self.d_off, n_items, s.size, K, self.dq, 3, self.d_query, self.d_end, self.start, self.dist, "end", self.pos)
        else:
            c.kmer_edist_start_async(ptr, s.size, K, self.dq, 3, self.d_query, self.d_end, n_items, self.start, self.dist)
        c.sync()
        return self.start.cpu().numpy().view(np.uint64 if self.wide else np.uint32).astype(np.uint64), self.dist.cpu().numpy()


@pytest.mark.parametrize("kind", ["fixed", "ragged", "reference"])
def test_start_path(ctx, kind):
    import bitnuc_amd as bn
    P = StartPath(ctx, kind)
    assert P.owned.any() and not P.owned.all()
    want = P.want(P.good)
    # ACCEPT
    for case in ("upper", "lower", "mixed"):
        got = P.run(al.recase(P.good, case, seed=5))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case
    # REJECT
    owned_pos = np.nonzero(P.owned)[0]
    cases = 0
    for byte, pos, region in al.reject_plan(P.regions):
        s = P.good.copy()
        s[pos] = byte
        later = owned_pos[owned_pos > pos]
        if later.size:
            s[int(later[(cases * 7) % later.size])] = al.other_class(byte, cases)  # a later invalid byte of the other class never wins
        with pytest.raises(bn.NucleotideError) as ei:
            P.run(s)
        assert (ei.value.byte, ei.value.index) == (byte, pos), (al.describe(byte), pos, region, ei.value.byte, ei.value.index)
        del ei
        ctx.sync()  # reported once
        cases += 1
    assert cases == 4 * len(al.INVALID)
    got = P.run(P.good)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # IGNORE: every byte the call does not own, and the bytes around the buffer, take every value
    for b in range(256):
        s = np.where(P.owned, P.good, np.uint8(b)).astype(np.uint8)
        got = P.run(s, around=b)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), al.describe(b)
