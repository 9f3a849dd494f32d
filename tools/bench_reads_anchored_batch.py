"""The anchored best match and runner-up per read of a RAGGED batch (bitnuc_reads_hdist_anchored_batch[_packed]_async; reads_anchored_kernel under its
ragged layout policy) against the fixed-length anchored form and against today's equal-result route for a ragged batch.  One process.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE) as two batches of --count reads:
  equal    every read 150 bases: the new form against bitnuc_reads_hdist_anchored[_packed]_async with the same answers (START lo .. hi as it stands; END
           e_lo .. e_hi as pos_lo = 150 - k - e_hi, pos_hi = 150 - k - e_lo) -- what the per-lane table loads, lengths and start values cost
  ragged   lengths uniform in [100, 200] (the last read takes up the rest): the new form against the route a caller has today -- a device gather of
           every read's span into a compact fixed-length batch (an index tensor built from the offsets table, one torch gather) and
           bitnuc_reads_hdist_anchored_async on it; packed: the same gather, encode_fixed_dev of the compact batch, and
           bitnuc_reads_hdist_anchored_packed_async (a caller that holds only packed words has no device route at all)
k in {16, 31}; 1 or 4 offsets; both anchors; Q in {1, 8, 64, 512} queries, half of them windows of reads at an admissible offset and half random; ASCII
bytes and packed words; all six outputs.  Per point, three alternating queues of each form, timed as bench.py times its config-5 block (sustained bursts
of back-to-back calls, timed_sustained).  Reported: the medians, each form's own spread over its three queues ((max - min) / median), new / other, and
whether the difference exceeds the two spreads added together.  The six arrays are compared with tests/reads_anchored_batch_oracle.py on the first
--sample reads and with the other form's on all reads.

    python tools/bench_reads_anchored_batch.py [--out FILE] [--ks 16,31] [--offsets 1,4] [--qs 1,8,64,512] [--count 6666667] [--sample 256]   one JSON document
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench import timed_sustained  # noqa: E402

SEED = 0xB17C0DE
READ_LEN = 150


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--offsets", default="1,4")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=256)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_anchored_batch_oracle as rab
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    count = args.count
    n = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    ctx.sync()
    rng = np.random.default_rng(2031)
    ragged = rng.integers(100, 201, size=count).astype(np.int64)
    ragged[-1] = 0
    rest = n - int(ragged.sum())
    while rest < 100 or rest > 200:  # the last read takes up the rest: pull it into the range by moving bases to or from other reads
        i = int(rng.integers(0, count - 1))
        step = 1 if rest > 200 else -1
        if 100 <= ragged[i] + step <= 200:
            ragged[i] += step
            rest -= step
    ragged[-1] = rest
    batches = {}
    for name, lengths in (("equal", np.full(count, READ_LEN, dtype=np.int64)), ("ragged", ragged)):
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lengths).astype(np.uint64)
        assert int(off[-1]) == n
        wtab = np.zeros(count + 1, dtype=np.uint64)
        wtab[1:] = np.cumsum((lengths + 31) // 32).astype(np.uint64)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_wtab = torch.from_numpy(wtab.view(np.int64)).to(dev)
        words = torch.zeros(int(wtab[-1]), dtype=torch.int64, device=dev)
        ctx.encode_batch_dev(ref, d_off, d_wtab, count, int(wtab[-1]), words)
        ctx.sync()
        batches[name] = dict(lengths=lengths, off=off, wtab=wtab, d_off=d_off, d_wtab=d_wtab, words=words, d_len=torch.from_numpy(lengths).to(dev),
                             head=ref[:int(off[sample])].cpu().numpy())
    doc = {"reads": count, "bases": n, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "ragged_lengths": [100, 200], "runs": []}
    types = (torch.int32, torch.int32, torch.uint8)
    six = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    alt = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    fixed_words = torch.zeros(count * ((READ_LEN + 31) // 32), dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, fixed_words)
    ctx.sync()
    assert torch.equal(fixed_words, batches["equal"]["words"])  # 150-base reads: encode_batch's layout is encode_fixed's
    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            for noff in [int(x) for x in args.offsets.split(",")]:
                span = noff + k - 1
                swpr = (span + 31) // 32
                for anchor in ("start", "end"):
                    for bname, b in batches.items():
                        lengths, d_off, d_wtab = b["lengths"], b["d_off"], b["d_wtab"]
                        first = np.zeros(count, dtype=np.int64) if anchor == "start" else lengths - k - (noff - 1)  # every read holds all offsets
                        qs = []
                        for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, noff, size=(nq + 1) // 2)):
                            at = int(b["off"][int(r)]) + int(first[int(r)]) + int(p)
                            h = ref[at:at + k].cpu().numpy()
                            qs.append(int(sum(int(((x >> 1) ^ (x >> 2)) & 3) << (2 * i) for i, x in enumerate(h))))
                        qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
                        queries = np.array(qs, dtype=np.uint64)
                        dq = torch.from_numpy(queries.view(np.int64)).to(dev)
                        want = rab.reads_anchored_batch(b["head"], b["off"][:sample + 1], k, queries, anchor, 0, noff - 1)
                        d_first = torch.from_numpy(first).to(dev)
                        for form in ("ascii", "packed"):
                            if form == "ascii":
                                new = lambda i: ctx.reads_hdist_anchored_batch_async(ref, d_off, count, n, k, dq, nq, *six[i & 1], pos_lo=0, pos_hi=noff - 1, anchor=anchor)
                            else:
                                new = lambda i: ctx.reads_hdist_anchored_batch_packed_async(b["words"], d_wtab, d_off, count, int(b["wtab"][-1]), k, dq, nq, *six[i & 1],
                                                                                            pos_lo=0, pos_hi=noff - 1, anchor=anchor)
                            if bname == "equal":  # the fixed form on the same reads
                                lo = 0 if anchor == "start" else READ_LEN - k - (noff - 1)
                                hi = noff - 1 if anchor == "start" else READ_LEN - k
                                if form == "ascii":
                                    other = lambda i: ctx.reads_hdist_anchored_async(ref, READ_LEN, count, k, dq, nq, *alt[i & 1], pos_lo=lo, pos_hi=hi)
                                else:
                                    other = lambda i: ctx.reads_hdist_anchored_packed_async(fixed_words, READ_LEN, count, k, dq, nq, *alt[i & 1], pos_lo=lo, pos_hi=hi)
                                shift = None
                            else:  # the gather route: the index tensor from the table, one gather, (the encode,) the fixed form on the compact batch
                                cwords = [torch.zeros(count * swpr, dtype=torch.int64, device=dev) for _ in range(2)]
                                cols = torch.arange(span, dtype=torch.int64, device=dev)

                                def other(i, form=form, cwords=cwords, cols=cols):
                                    starts = d_off[:-1] + (0 if anchor == "start" else b["d_len"] - (k + noff - 1))
                                    compact = torch.take(ref, starts[:, None] + cols[None, :])  # (count, span), from torch's caching allocator, stream-ordered
                                    if form == "ascii":
                                        ctx.reads_hdist_anchored_async(compact, span, count, k, dq, nq, *alt[i & 1], pos_lo=0, pos_hi=noff - 1)
                                    else:
                                        ctx.encode_fixed_dev(compact, span, span, count, cwords[i & 1])
                                        ctx.reads_hdist_anchored_packed_async(cwords[i & 1], span, count, k, dq, nq, *alt[i & 1], pos_lo=0, pos_hi=noff - 1)
                                shift = d_first.to(torch.int32)
                            for a in six[0] + alt[0]:
                                a.fill_(0x5A)
                            new(0)
                            other(0)
                            ctx.sync()
                            got = [a[:sample].cpu().numpy() for a in six[0]]
                            equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
                            equal_other = True
                            for j, (x, y) in enumerate(zip(six[0], alt[0])):
                                if j % 3 == 1 and shift is not None:  # positions: the route's count from the span's first base
                                    y = torch.where(y == -1, y, y + shift)
                                equal_other = equal_other and bool(torch.equal(x, y))
                            burst, rounds = (8, 3) if nq <= 64 else (4, 2)
                            runs = {"new": [], "other": []}
                            for _ in range(3):  # alternating queues
                                runs["new"].append(timed_sustained(torch, stream, new, burst=burst, rounds=rounds))
                                runs["other"].append(timed_sustained(torch, stream, other, burst=burst, rounds=rounds))
                            ctx.sync()
                            med = {name: statistics.median(v) for name, v in runs.items()}
                            gap = abs(med["other"] - med["new"])
                            noise = spread(runs["new"]) * med["new"] + spread(runs["other"]) * med["other"]
                            run = {"batch": bname, "against": "fixed form" if bname == "equal" else "gather route", "k": k, "n_queries": nq, "offsets": noff,
                                   "anchor": anchor, "span": span, "form": form, "equal_to_oracle_on_sample": equal_oracle, "equal_to_other": equal_other,
                                   "new_ms": round(med["new"], 4), "new_runs_ms": [round(x, 4) for x in runs["new"]], "new_spread": round(spread(runs["new"]), 4),
                                   "other_ms": round(med["other"], 4), "other_runs_ms": [round(x, 4) for x in runs["other"]],
                                   "other_spread": round(spread(runs["other"]), 4), "new_over_other": round(med["new"] / med["other"], 4),
                                   "verdict": "within the spreads" if gap <= noise else ("new faster" if med["new"] < med["other"] else "new slower")}
                            doc["runs"].append(run)
                            print(json.dumps(run), flush=True)
                            if bname != "equal":
                                del cwords, cols, other
                        del dq
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["equal_to_other"] for r in doc["runs"])
    doc["new_slower_points"] = [{key: r[key] for key in ("batch", "k", "n_queries", "offsets", "anchor", "form", "new_over_other")} for r in doc["runs"]
                                if r["verdict"] == "new slower"]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
