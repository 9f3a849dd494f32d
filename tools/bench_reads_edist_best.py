"""The indel-tolerant best match per read over the WHOLE read (bitnuc_reads_edist_best[_packed]_async, _best_batch[_packed]_async and the pattern twins;
reads_edist_best_kernel) against the anchored edit-distance form at span 64 -- the same step, one piece, the parent's kernel -- and against the whole-read
Hamming forms on the same arguments (another answer: the price of indel tolerance).  One process.  No equal-result route exists for reads above 64 bases.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE) as two batches of --count reads: every read 150 bases (fixed layout, and the ragged layout on equal
lengths), and lengths uniform in [100, 200] (the last read takes up the rest).  k in {16, 31}; Q in {1, 8, 64, 512} queries, half of them windows of reads
and half random; ASCII bytes and packed words; exact queries and their singleton patterns; all six outputs.  Per point, three alternating queues of each
form, timed as bench.py times its config-5 block (timed_sustained).  Reported per point:
  1. fixed: the time per (read, query, base) over that of bitnuc_reads_edist_anchored*_async at span 64 on the same reads (pos 0 .. 64 - k).  The step is
     the same 20 vector instructions; at Q >= 64 the ratio is held against 1 + PIECE_VALU / 5120 + the anchored form's own spread in that run (PIECE_VALU:
     the vector instructions of one piece's load, validate and encode in the shipped disassembly; 5120 = 64 steps x 4 queries x 20)
  2. ragged on equal lengths over fixed: the bound is 1 + 1.25 / 20 + the fixed form's spread
  3. ragged on 100 .. 200 bases over ragged on equal lengths, next to the prediction from the length distribution: the loop follows the longest read of
     each wave of 64 consecutive reads, masked steps cost 21.25 / 20 of unmasked ones
  4. over bitnuc_reads_hdist_best[_batch]*_async on the same arguments
The six arrays are compared with tests/reads_edist_best_oracle.py (the numpy DP) on the first --sample reads, the pattern twin with the exact form on all
reads.

    python tools/bench_reads_edist_best.py [--out FILE] [--ks 16,31] [--qs 1,8,64,512] [--count 6666667] [--sample 16]   one JSON document
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
ANCHOR_SPAN = 64
STEP_VALU = 20.0    # vector instructions per (read, query, base) of the unmasked loop (scan_edist_device.h)
MASK_VALU = 1.25    # what the masked loop adds per (query, step)
PIECE_VALU = {"ascii": 252.0, "packed": 13.0}  # one piece's load, validate and encode (DESIGN 3.4 has the count from the disassembly)


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=16)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_edist_best_oracle as bo
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
        return dict(lengths=lengths, off=off, wtab=wtab, d_off=d_off, d_wtab=d_wtab, words=words, head=ref[:int(off[sample])].cpu().numpy())

    equal, rag = make_batch(np.full(count, READ_LEN, dtype=np.int64)), make_batch(ragged)
    full = ragged[:count - count % 64].reshape(-1, 64)
    wave_max = np.concatenate([full.max(axis=1), ragged[count - count % 64:].max(keepdims=True)]) if count % 64 else full.max(axis=1)
    wave_n = np.concatenate([np.full(full.shape[0], 64), [count % 64]]) if count % 64 else np.full(full.shape[0], 64)
    predicted = float((wave_max * wave_n).sum()) / float(n) * (STEP_VALU + MASK_VALU) / STEP_VALU  # lane-steps run over lane-steps of the equal batch
    doc = {"reads": count, "bases": n, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "ragged_lengths": [100, 200], "anchored_span": ANCHOR_SPAN, "step_valu_per_query": STEP_VALU, "masked_loop_adds_valu_per_query": MASK_VALU,
           "piece_valu": PIECE_VALU, "predicted_ragged_over_equal": round(predicted, 4), "runs": []}
    types = (torch.int32, torch.int32, torch.uint8)
    outs = {name: [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)] for name in ("fixed", "req", "rag", "anch", "ham", "twin")}
    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            qs = []
            for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, 100 - k + 1, size=(nq + 1) // 2)):
                at = int(rag["off"][int(r)]) + int(p)
                h = ref[at:at + k].cpu().numpy()
                qs.append(int(sum(int(((x >> 1) ^ (x >> 2)) & 3) << (2 * i) for i, x in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            dqs = {"exact": torch.from_numpy(queries.view(np.int64)).to(dev), "pattern": torch.from_numpy(rp.singletons(queries, k).view(np.int32).copy()).to(dev)}
            want_eq = bo.reads_edist_best(equal["head"], READ_LEN, sample, k, queries)
            want_rag = bo.reads_edist_best_batch(rag["head"], rag["off"][:sample + 1], k, queries)
            for form in ("ascii", "packed"):
                pk = "" if form == "ascii" else "_packed"
                for kind, dq in dqs.items():
                    stem = "reads_edist" if kind == "exact" else "reads_pattern_edist"
                    hstem = "reads_hdist_best" if kind == "exact" else "reads_pattern_best"
                    ffix, frag = getattr(ctx, stem + "_best" + pk + "_async"), getattr(ctx, stem + "_best_batch" + pk + "_async")
                    fanch = getattr(ctx, stem + "_anchored" + pk + "_async")
                    fham, fhamb = getattr(ctx, hstem + pk + "_async"), getattr(ctx, hstem + "_batch" + pk + "_async")
                    src = ref if form == "ascii" else equal["words"]

                    def batch_head(b):
                        return (ref, b["d_off"], count, n) if form == "ascii" else (b["words"], b["d_wtab"], b["d_off"], count, int(b["wtab"][-1]))
                    calls = {
                        "fixed": lambda i: ffix(src, READ_LEN, count, k, dq, nq, *outs["fixed"][i & 1]),
                        "req": lambda i: frag(*batch_head(equal), k, dq, nq, *outs["req"][i & 1]),
                        "rag": lambda i: frag(*batch_head(rag), k, dq, nq, *outs["rag"][i & 1]),
                        "anch": lambda i: fanch(src, READ_LEN, count, k, dq, nq, *outs["anch"][i & 1], pos_lo=0, pos_hi=ANCHOR_SPAN - k),
                        "ham": lambda i: fham(src, READ_LEN, count, k, dq, nq, *outs["ham"][i & 1][:3]),
                        "ham_rag": lambda i: fhamb(*batch_head(rag), k, dq, nq, *outs["ham"][i & 1][:3]),
                    }
                    for name in ("fixed", "req", "rag"):
                        for a in outs[name][0]:
                            a.fill_(0x5A)
                        calls[name](0)
                    ctx.sync()
                    got_eq = [a[:sample].cpu().numpy() for a in outs["fixed"][0]]
                    got_rag = [a[:sample].cpu().numpy() for a in outs["rag"][0]]
                    equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got_eq, want_eq)) and \
                        all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got_rag, want_rag))
                    ragged_equals_fixed = all(bool(torch.equal(x, y)) for x, y in zip(outs["fixed"][0], outs["req"][0]))
                    twin_equal = None
                    if kind == "pattern":  # against the exact form on all reads
                        twin = getattr(ctx, "reads_edist_best" + pk + "_async")
                        twin(src, READ_LEN, count, k, dqs["exact"], nq, *outs["twin"][0])
                        ctx.sync()
                        twin_equal = all(bool(torch.equal(x, y)) for x, y in zip(outs["fixed"][0], outs["twin"][0]))
                    burst, rounds = (8, 3) if nq <= 8 else ((2, 1) if nq <= 64 else (1, 1))
                    runs = {name: [] for name in calls}
                    for _ in range(3):  # alternating queues
                        for name, fn in calls.items():
                            runs[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                    ctx.sync()
                    med = {name: statistics.median(v) for name, v in runs.items()}
                    per_step = {"fixed": med["fixed"] / READ_LEN, "anch": med["anch"] / ANCHOR_SPAN}
                    run = {"k": k, "n_queries": nq, "form": form, "queries": kind, "equal_to_oracle_on_sample": equal_oracle, "ragged_on_equal_lengths_equals_fixed": ragged_equals_fixed,
                           "pattern_twin_equals_exact": twin_equal}
                    for name in calls:
                        run[name + "_ms"] = round(med[name], 4)
                        run[name + "_runs_ms"] = [round(x, 4) for x in runs[name]]
                        run[name + "_spread"] = round(spread(runs[name]), 4)
                    run["ps_per_read_query_base"] = round(med["fixed"] * 1e9 / (count * nq * READ_LEN), 4)
                    run["anchored_ps_per_read_query_base"] = round(med["anch"] * 1e9 / (count * nq * ANCHOR_SPAN), 4)
                    run["step_over_anchored_step"] = round(per_step["fixed"] / per_step["anch"], 4)
                    run["ragged_equal_over_fixed"] = round(med["req"] / med["fixed"], 4)
                    run["ragged_over_ragged_equal"] = round(med["rag"] / med["req"], 4)
                    run["over_hamming_fixed"] = round(med["fixed"] / med["ham"], 4)
                    run["over_hamming_ragged"] = round(med["rag"] / med["ham_rag"], 4)
                    if nq >= 64:
                        run["step_bound"] = round(1.0 + PIECE_VALU[form] / (64 * 4 * STEP_VALU) + spread(runs["anch"]), 4)
                        run["step_within_bound"] = run["step_over_anchored_step"] <= run["step_bound"]
                        run["ragged_equal_bound"] = round(1.0 + MASK_VALU / STEP_VALU + spread(runs["fixed"]), 4)
                        run["ragged_equal_within_bound"] = run["ragged_equal_over_fixed"] <= run["ragged_equal_bound"]
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
            del dqs
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["ragged_on_equal_lengths_equals_fixed"] and r["pattern_twin_equals_exact"] is not False for r in doc["runs"])
    doc["outside_bound_points"] = [{key: r[key] for key in ("k", "n_queries", "form", "queries", "step_over_anchored_step", "step_bound", "ragged_equal_over_fixed",
                                                               "ragged_equal_bound")} for r in doc["runs"]
                                   if r.get("step_within_bound") is False or r.get("ragged_equal_within_bound") is False]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
