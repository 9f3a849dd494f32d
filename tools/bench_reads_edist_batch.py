"""The indel-tolerant anchored match per read of a RAGGED batch (bitnuc_reads_edist_anchored_batch[_packed]_async and the pattern twins; reads_edist_kernel
under its ragged layout policy) against the fixed-length edit-distance form and against today's equal-result route for a ragged batch.  One process.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE) as two batches of --count reads:
  equal    every read 150 bases: the new form against bitnuc_reads_edist_anchored[_packed]_async with the same answers (START lo .. hi as it stands; END
           e_lo .. e_hi as pos_lo = 150 - k - e_hi, pos_hi = 150 - k - e_lo) -- the price of the ragged layout: the per-lane table loads and the
           wave-uniform test in front of the fixed form's loop (every lane has the full span, so the masked loop never runs).  At Q >= 64 the ratio is
           held against 1 + MASK_VALU / STEP_VALU + the fixed form's own spread in that run (MASK_VALU: the vector instructions the masked loop adds per
           (query, step), from the disassembly: the bound covers a batch that took the masked loop throughout)
  ragged   lengths uniform in [100, 200] (the last read takes up the rest): the new form against the route a caller has today -- a device gather of
           every read's span into a compact fixed-length batch (an index tensor built from the offsets table, one torch gather) and
           bitnuc_reads_edist_anchored_async on it, the ends re-based; packed: the same gather, encode_fixed_dev of the compact batch, and
           bitnuc_reads_edist_anchored_packed_async.  Every read there has the full span, so the answers are equal.  At Q >= 64 the recurrence dominates
           both routes and a ratio near 1 is the expected outcome
  mixed    (--mixed) the ragged batch with every fourth read cut to k + 1 bases and its other bases given to the next read: every wave mixes full
           and short spans and takes the masked loop; against the new form on the ragged batch, where every wave takes the fixed form's loop (another
           answer: the ratio is what the masked loop costs)
k = 16 with four offsets and k = 31 with eight; both anchors; Q in {1, 8, 64, 512} queries, half of them windows of reads at an admissible offset and
half random; ASCII bytes and packed words; exact queries and their singleton patterns; all six outputs.  Per point, three alternating queues of each
form, timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported: the medians, each form's own
spread over its three queues ((max - min) / median), new / other, and whether the difference exceeds the two spreads added together.  The six arrays
are compared with tests/reads_edist_batch_oracle.py on the first --sample reads and with the other form's on all reads.

    python tools/bench_reads_edist_batch.py [--out FILE] [--points 16:4,31:8] [--qs 1,8,64,512] [--count 6666667] [--sample 128] [--mixed]   one JSON document
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
STEP_VALU = 20.0   # vector instructions per (read, query, span base) of the fixed loop (scan_edist_device.h)
MASK_VALU = 1.25   # what the masked loop adds: four v_cndmask (Eq behind the span -> 0) and one v_cmp per step of four interleaved queries


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default="16:4,31:8", help="k:offsets pairs")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=128)
    ap.add_argument("--mixed", action="store_true", help="also the masked loop's price: a batch in which every fourth read has a short span")
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_edist_batch_oracle as ebo
    import reads_pattern_oracle as rp
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

    def make_batch(lengths):
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
        return dict(lengths=lengths, off=off, wtab=wtab, d_off=d_off, d_wtab=d_wtab, words=words, d_len=torch.from_numpy(lengths).to(dev),
                    head=ref[:int(off[sample])].cpu().numpy())

    batches = {"equal": make_batch(np.full(count, READ_LEN, dtype=np.int64)), "ragged": make_batch(ragged)}
    doc = {"reads": count, "bases": n, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "ragged_lengths": [100, 200], "step_valu_per_query": STEP_VALU, "masked_loop_adds_valu_per_query": MASK_VALU, "runs": []}
    types = (torch.int32, torch.int32, torch.uint8)
    six = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    alt = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    fixed_words = torch.zeros(count * ((READ_LEN + 31) // 32), dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, fixed_words)
    ctx.sync()
    assert torch.equal(fixed_words, batches["equal"]["words"])  # 150-base reads: encode_batch's layout is encode_fixed's
    for k, noff in [tuple(int(x) for x in p.split(":")) for p in args.points.split(",")]:
        span = noff + k - 1
        if args.mixed:  # every fourth read k + 1 bases (two offsets), the bases it gives up go to the next read: the same count and total
            mixed = ragged.copy()
            mixed[1::4][:len(mixed[0:-1:4])] += mixed[0:-1:4] - (k + 1)
            mixed[0:-1:4] = k + 1
            batches["mixed"] = make_batch(mixed)
        swpr = (span + 31) // 32
        for nq in [int(x) for x in args.qs.split(",")]:
            for anchor in ("end", "start"):
                for bname, b in batches.items():
                    lengths, d_off, d_wtab = b["lengths"], b["d_off"], b["d_wtab"]
                    first = np.zeros(count, dtype=np.int64) if anchor == "start" else np.maximum(lengths - k - (noff - 1), 0)
                    qs = []
                    for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, noff, size=(nq + 1) // 2)):
                        r += int(lengths[int(r)] < span)  # (the mixed batch: a cut read's neighbour holds all offsets)
                        at = int(b["off"][int(r)]) + int(first[int(r)]) + int(p)
                        h = ref[at:at + k].cpu().numpy()
                        qs.append(int(sum(int(((x >> 1) ^ (x >> 2)) & 3) << (2 * i) for i, x in enumerate(h))))
                    qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
                    queries = np.array(qs, dtype=np.uint64)
                    dqs = {"exact": torch.from_numpy(queries.view(np.int64)).to(dev), "pattern": torch.from_numpy(rp.singletons(queries, k).view(np.int32).copy()).to(dev)}
                    want = ebo.reads_edist_batch(b["head"], b["off"][:sample + 1], k, queries, anchor, 0, noff - 1)
                    d_first = torch.from_numpy(first).to(dev)
                    for kind, dq in dqs.items():
                        stem = "reads_edist_anchored" if kind == "exact" else "reads_pattern_edist_anchored"
                        for form in ("ascii", "packed"):
                            fnew = getattr(ctx, stem + "_batch" + ("" if form == "ascii" else "_packed") + "_async")
                            ffix = getattr(ctx, stem + ("" if form == "ascii" else "_packed") + "_async")
                            if form == "ascii":
                                new = lambda i: fnew(ref, d_off, count, n, k, dq, nq, *six[i & 1], pos_lo=0, pos_hi=noff - 1, anchor=anchor)
                            else:
                                new = lambda i: fnew(b["words"], d_wtab, d_off, count, int(b["wtab"][-1]), k, dq, nq, *six[i & 1], pos_lo=0, pos_hi=noff - 1, anchor=anchor)
                            if bname == "equal":  # the fixed form on the same reads
                                lo = 0 if anchor == "start" else READ_LEN - k - (noff - 1)
                                hi = noff - 1 if anchor == "start" else READ_LEN - k
                                src = ref if form == "ascii" else fixed_words
                                other = lambda i: ffix(src, READ_LEN, count, k, dq, nq, *alt[i & 1], pos_lo=lo, pos_hi=hi)
                                shift = None
                            elif bname == "mixed":  # the new form on the ragged batch: the fixed form's loop in every wave
                                g = batches["ragged"]
                                if form == "ascii":
                                    other = lambda i: fnew(ref, g["d_off"], count, n, k, dq, nq, *alt[i & 1], pos_lo=0, pos_hi=noff - 1, anchor=anchor)
                                else:
                                    other = lambda i: fnew(g["words"], g["d_wtab"], g["d_off"], count, int(g["wtab"][-1]), k, dq, nq, *alt[i & 1], pos_lo=0,
                                                           pos_hi=noff - 1, anchor=anchor)
                                shift = None
                            else:  # the gather route: the index tensor from the table, one gather, (the encode,) the fixed form on the compact batch
                                cwords = [torch.zeros(count * swpr, dtype=torch.int64, device=dev) for _ in range(2)]
                                cols = torch.arange(span, dtype=torch.int64, device=dev)

                                def other(i, form=form, cwords=cwords, cols=cols, ffix=ffix, dq=dq):
                                    starts = d_off[:-1] + (0 if anchor == "start" else b["d_len"] - (k + noff - 1))
                                    compact = torch.take(ref, starts[:, None] + cols[None, :])  # (count, span), from torch's caching allocator, stream-ordered
                                    if form == "ascii":
                                        ffix(compact, span, count, k, dq, nq, *alt[i & 1], pos_lo=0, pos_hi=noff - 1)
                                    else:
                                        ctx.encode_fixed_dev(compact, span, span, count, cwords[i & 1])
                                        ffix(cwords[i & 1], span, count, k, dq, nq, *alt[i & 1], pos_lo=0, pos_hi=noff - 1)
                                shift = d_first.to(torch.int32)
                            for a in six[0] + alt[0]:
                                a.fill_(0x5A)
                            new(0)
                            other(0)
                            ctx.sync()
                            got = [a[:sample].cpu().numpy() for a in six[0]]
                            equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
                            equal_other = True
                            for j, (x, y) in enumerate(zip(six[0], alt[0]) if bname != "mixed" else ()):
                                if j % 3 == 1 and shift is not None:  # ends: the route's count from the span's first base
                                    y = torch.where(y == -1, y, y + shift)
                                equal_other = equal_other and bool(torch.equal(x, y))
                            burst, rounds = (8, 3) if nq <= 64 else (2, 1)
                            runs = {"new": [], "other": []}
                            for _ in range(3):  # alternating queues
                                runs["new"].append(timed_sustained(torch, stream, new, burst=burst, rounds=rounds))
                                runs["other"].append(timed_sustained(torch, stream, other, burst=burst, rounds=rounds))
                            ctx.sync()
                            med = {name: statistics.median(v) for name, v in runs.items()}
                            gap = abs(med["other"] - med["new"])
                            noise = spread(runs["new"]) * med["new"] + spread(runs["other"]) * med["other"]
                            against = {"equal": "fixed form", "ragged": "gather route", "mixed": "new form on the ragged batch"}[bname]
                            run = {"batch": bname, "against": against, "k": k, "n_queries": nq, "offsets": noff, "anchor": anchor, "span": span, "form": form, "queries": kind, "equal_to_oracle_on_sample": equal_oracle, "equal_to_other": equal_other,
                                   "new_ms": round(med["new"], 4), "new_runs_ms": [round(x, 4) for x in runs["new"]], "new_spread": round(spread(runs["new"]), 4),
                                   "other_ms": round(med["other"], 4), "other_runs_ms": [round(x, 4) for x in runs["other"]],
                                   "other_spread": round(spread(runs["other"]), 4), "new_over_other": round(med["new"] / med["other"], 4),
                                   "verdict": "within the spreads" if gap <= noise else ("new faster" if med["new"] < med["other"] else "new slower")}
                            if bname == "equal" and nq >= 64:
                                run["bound"] = round(1.0 + MASK_VALU / STEP_VALU + spread(runs["other"]), 4)
                                run["within_bound"] = run["new_over_other"] <= run["bound"]
                            doc["runs"].append(run)
                            print(json.dumps(run), flush=True)
                            if bname == "ragged":
                                del cwords, cols, other
                    del dqs
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r.get("equal_to_other", True) for r in doc["runs"])
    doc["new_slower_points"] = [{key: r[key] for key in ("batch", "k", "n_queries", "offsets", "anchor", "form", "queries", "new_over_other")} for r in doc["runs"]
                                if r.get("verdict") == "new slower"]
    doc["outside_bound_points"] = [{key: r[key] for key in ("k", "n_queries", "offsets", "anchor", "form", "queries", "new_over_other", "bound")} for r in doc["runs"]
                                   if r.get("within_bound") is False]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
