"""All 256 byte values in and beside the ASCII input of the two ASCII paths of reads_edist_adapter_kernel (-m gpu): bitnuc_reads_edist_adapter_async (fixed)
and bitnuc_reads_edist_adapter_batch_async (ragged), in the manner of tests/test_gpu_edist_start_alphabet.py with tests/alphabet.py's classes and reject_plan.

OWNED positions are the validated bytes as the header block states them: every byte of every read of at least k bases, nothing else -- not a byte of a
ragged read shorter than k, not the bytes around the buffer.  (The cut's backward walk re-reads bytes the forward walk validated; it reports nothing.)
ACCEPT: upper, lower and mixed case give the oracle's result.  REJECT: each of the 248 invalid values once at each byte lane of a dword (992 cases per
path, rotating over the path's regions: a read's first bytes, the bytes around a piece boundary, its last bytes, the rest); the error is the first invalid
OWNED byte in buffer order -- a later one of the other class never wins --, the next sync is clean, and a clean call follows the sweep.  IGNORE: every byte
that is not owned takes each of the 256 values: the call succeeds with the oracle's result."""
import numpy as np
import pytest

import alphabet as al
import reads_batch_oracle as rb
import reads_best_oracle as ro
import reads_edist_adapter_oracle as ao

pytestmark = pytest.mark.gpu

K = 16
RULE = (3, 1, 10)
PAD = 67  # bytes around the input in its device buffer: not owned


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


class AdapterPath:
    """one ASCII path: the clean input, the validated bytes and the call on a device buffer"""

    def __init__(self, ctx, kind):
        import torch
        rng = np.random.default_rng({"fixed": 21, "ragged": 22}[kind])
        self.ctx, self.kind, self.torch = ctx, kind, torch
        self.queries = ro.random_queries(rng, 3, K)
        self.dq = _dev(self.queries)
        count = 200
        lens = np.full(count, 100) if kind == "fixed" else rng.integers(0, 201, size=count)
        if kind == "ragged":
            lens[:6] = [K - 1, K, 0, 3, 64, 129]
        self.lens = [int(x) for x in lens]
        self.off = rb.offsets_of(lens)
        total = int(self.off[-1])
        self.good = al.bases(rng, total, "upper")
        for r, ln in enumerate(self.lens):  # every other read of k bases ends with a prefix of an adapter: the cut's walk runs
            if ln >= K and r % 2:
                i = int(rng.integers(3, K + 1))
                self.good[int(self.off[r + 1]) - i:int(self.off[r + 1])] = ro.LUT[np.asarray(ro.query_codes(self.queries[r % 3], K), dtype=np.int64)[:i]]
        owned = np.zeros(total, dtype=bool)
        first, edge, last, rest = [], [], [], []
        for r, ln in enumerate(self.lens):
            if ln < K:
                continue
            lo = int(self.off[r])
            owned[lo:lo + ln] = True
            pos = set(range(lo, lo + ln))
            f, la = set(range(lo, lo + 4)), set(range(lo + ln - 4, lo + ln)) - set(range(lo, lo + 4))
            e = (set(range(lo + 60, lo + 68)) & pos) - f - la
            first += sorted(f)
            last += sorted(la)
            edge += sorted(e)
            rest += sorted(pos - f - la - e)
        self.owned = owned
        self.regions = [("a read's first bytes", first), ("around a piece boundary", edge), ("a read's last bytes", last), ("the rest", rest)]
        self.buf = torch.zeros(total + 2 * PAD, dtype=torch.uint8, device="cuda:0")
        self.d_off = _dev(self.off)
        self.w = [torch.zeros(count, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        self.d = [torch.zeros(count, dtype=torch.uint8, device="cuda:0") for _ in range(2)]

    def want(self, s):
        return ao.reads_edist_adapter_batch(s, self.off, K, self.queries, *RULE)

    def run(self, s, around=0):
        """the call on the bytes s (the bytes around them: `around`) -> the five outputs after a sync, which raises the call's error"""
        torch, c = self.torch, self.ctx
        self.buf.fill_(around)
        self.buf[PAD:PAD + s.size] = torch.from_numpy(s)
        for a in self.w + self.d:
            a.fill_(0x5A)
        ptr = self.buf.data_ptr() + PAD
        if self.kind == "fixed":
            c.reads_edist_adapter_async(ptr, 100, len(self.lens), K, self.dq, 3, *self.w, *self.d, *RULE)
        else:
            c.reads_edist_adapter_batch_async(ptr, self.d_off, len(self.lens), s.size, K, self.dq, 3, *self.w, *self.d, *RULE)
        c.sync()
        return tuple(a.cpu().numpy().view(np.uint32) for a in self.w) + tuple(a.cpu().numpy() for a in self.d)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_adapter_path(ctx, kind):
    import bitnuc_amd as bn
    P = AdapterPath(ctx, kind)
    assert P.owned.any() and (kind == "fixed" or not P.owned.all())
    want = P.want(P.good)
    assert (want[0] != ao.NO_U32).sum() > 50
    # ACCEPT
    for case in ("upper", "lower", "mixed"):
        assert _same(P.run(al.recase(P.good, case, seed=5)), want), case
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
    assert _same(P.run(P.good), want)
    # IGNORE: every byte the call does not own, and the bytes around the buffer, take every value
    for b in range(256):
        s = np.where(P.owned, P.good, np.uint8(b)).astype(np.uint8)
        assert _same(P.run(s, around=b), want), al.describe(b)
