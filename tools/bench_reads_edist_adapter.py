"""The 3' adapter per read (bitnuc_reads_edist_adapter*_async; reads_edist_adapter_kernel) against today's nearest route in the same queues.  One process.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE) as two batches of --count reads: every read 150 bases (the fixed forms) and lengths uniform in
[100, 200] (the ragged forms; the last read takes up the rest).  k in {16, 31}, Q in {1, 8, 64, 512} adapters (half of them cut from the reads, half
random), rate 1 / 10, min_overlap 3; ASCII bytes and packed words: the four _async forms.  Three alternating queues of each call per point, timed as
bench.py times its config-5 block (timed_sustained).
  The yardstick is the ROUTE: bitnuc_reads_edist_best*_async with the second triple NULL, followed by bitnuc_reads_edist_start*_async on its (query, end)
  with (START, 0) -- existing code, never the code under test.  It finds no overhangs, so it is a yardstick of COST only.
  The bound, from the shipped disassembly: the adapter call walks the read with the route's own step (STEP_VALU vector instructions per
  (read, query, base)), then decodes k - 1 prefix lengths per (read, query) at DECODE_VALU each, then walks backwards once per read as the route's second
  call does.  Fixed: route x (1 + DECODE_VALU (k - 1) / (STEP_VALU read_len)) + the route's own spread.  Ragged: the masked loop snapshots the column
  (SNAP_STEP_VALU a step against the route's MASK_STEP_VALU) and both run over the longest read of each wave of 64: route x (SNAP_STEP_VALU / MASK_STEP_VALU
  + DECODE_VALU (k - 1) / (MASK_STEP_VALU x that length's mean)) + spread.  Each point is reported as inside or outside its bound.
Every output of the adapter call is compared with tests/reads_edist_adapter_oracle.py on the first --sample reads; with min_overlap = k and rate 1 / 1 the
call must equal the route on ALL reads (the header's first identity).

    python tools/bench_reads_edist_adapter.py [--out FILE] [--ks 16,31] [--qs 1,8,64,512] [--count 6666667] [--sample 32]   one JSON document
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
MIN_OVERLAP, ERR_NUM, ERR_DEN = 3, 1, 10
STEP_VALU = 20.0        # the walk's vector instructions per (read, query, base): the route's and the adapter call's unmasked loops are the same 80 for four queries
MASK_STEP_VALU = 21.25  # the route's masked loop (ragged waves of unequal lengths): 85 for four queries
SNAP_STEP_VALU = 24.0   # the adapter call's masked loop with the column snapshot: 96 for four queries
DECODE_VALU = 9.0       # per (read, query, prefix length): 36 for four queries (two bit extracts, the distance, the candidate, the compare, the select, the minimum)


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def word_of(h):
    return int(sum(int(((x >> 1) ^ (x >> 2)) & 3) << (2 * i) for i, x in enumerate(h)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=32)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_edist_adapter_oracle as ao
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)
    count = args.count
    n = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, ref.numel(), SEED)
    ctx.sync()
    rng = np.random.default_rng(2531)
    ragged = rng.integers(100, 201, size=count).astype(np.int64)
    ragged[-1] = 0
    rest = n - int(ragged.sum())
    while rest < 100 or rest > 200:
        i = int(rng.integers(0, count - 1))
        step = 1 if rest > 200 else -1
        if 100 <= ragged[i] + step <= 200:
            ragged[i] += step
            rest -= step
    ragged[-1] = rest
    pad = (-count) % 64
    longest = float(np.concatenate([ragged, np.zeros(pad, dtype=np.int64)]).reshape(-1, 64).max(axis=1).mean())  # of a wave of 64 consecutive reads

    def make_batch(lengths):
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lengths).astype(np.uint64)
        wtab = np.zeros(count + 1, dtype=np.uint64)
        wtab[1:] = np.cumsum((lengths + 31) // 32).astype(np.uint64)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_wtab = torch.from_numpy(wtab.view(np.int64)).to(dev)
        words = torch.zeros(int(wtab[-1]), dtype=torch.int64, device=dev)
        ctx.encode_batch_dev(ref, d_off, d_wtab, count, int(wtab[-1]), words)
        ctx.sync()
        return dict(off=off, wtab=wtab, d_off=d_off, d_wtab=d_wtab, words=words, head=ref[:int(off[sample])].cpu().numpy())

    equal, rag = make_batch(np.full(count, READ_LEN, dtype=np.int64)), make_batch(ragged)
    doc = {"reads": count, "bases": n, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "ragged_lengths": [100, 200], "mean_longest_read_per_wave": round(longest, 2), "min_overlap": MIN_OVERLAP, "rate": [ERR_NUM, ERR_DEN],
           "yardstick": "bitnuc_reads_edist_best*_async (second triple NULL) followed by bitnuc_reads_edist_start*_async (START, 0)",
           "step_valu": STEP_VALU, "masked_step_valu_route": MASK_STEP_VALU, "masked_step_valu_adapter": SNAP_STEP_VALU, "decode_valu": DECODE_VALU, "runs": []}
    i32, u8 = torch.int32, torch.uint8
    five = [tuple(torch.zeros(count, dtype=t, device=dev) for t in (i32, i32, i32, u8, u8)) for _ in range(2)]
    fw = [tuple(torch.zeros(count, dtype=t, device=dev) for t in (i32, i32, u8)) for _ in range(2)]
    st = [(torch.zeros(count, dtype=i32, device=dev), torch.zeros(count, dtype=u8, device=dev)) for _ in range(2)]

    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            # half of the adapters are cut from the reads' last bases (overhangs and full copies exist), half are random
            cut = []
            for a in rng.integers(0, count - 1, size=(nq + 1) // 2):
                end = int(equal["off"][int(a) + 1])
                at = end - int(rng.integers(3, k + 1))
                cut.append(word_of(ref[at:at + k].cpu().numpy()))
            queries = np.array(cut + [int(x) for x in rng.integers(0, 2**62, size=nq // 2)], dtype=np.uint64)
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            for layout in ("fixed", "ragged"):
                b = equal if layout == "fixed" else rag
                want = ao.reads_edist_adapter_batch(b["head"], b["off"][:sample + 1], k, queries, MIN_OVERLAP, ERR_NUM, ERR_DEN)  # once for both forms
                for form in ("ascii", "packed"):
                    pk = "" if form == "ascii" else "_packed"
                    if layout == "fixed":
                        head = (ref if form == "ascii" else b["words"], READ_LEN, count)
                        adapter, best, start = (getattr(ctx, f"reads_edist_{w}{pk}_async") for w in ("adapter", "best", "start"))
                    else:
                        head = (ref, b["d_off"], count, n) if form == "ascii" else (b["words"], b["d_wtab"], b["d_off"], count, int(b["wtab"][-1]))
                        adapter, best, start = (getattr(ctx, f"reads_edist_{w}_batch{pk}_async") for w in ("adapter", "best", "start"))

                    def route(i):
                        best(*head, k, dq, nq, *fw[i & 1])
                        start(*head, k, dq, nq, fw[i & 1][0], fw[i & 1][1], *st[i & 1], "start", 0)

                    calls = {"adapter": lambda i: adapter(*head, k, dq, nq, *five[i & 1], MIN_OVERLAP, ERR_NUM, ERR_DEN), "route": route}
                    # the results: the oracle on a sample; the first identity on every read
                    calls["adapter"](0)
                    ctx.sync()
                    got = tuple(a[:sample].cpu().numpy().view(np.uint32 if a.dtype == i32 else np.uint8) for a in five[0])
                    ok_sample = all(np.array_equal(x, y) for x, y in zip(got, want))
                    found = int((five[0][0] != -1).sum().item())
                    overhangs = int(((five[0][3] != 255) & (five[0][3] < k)).sum().item())
                    adapter(*head, k, dq, nq, *five[1], k, 1, 1)
                    route(0)
                    ctx.sync()
                    ok_route = bool(torch.equal(five[1][0], fw[0][0]) and torch.equal(five[1][2], fw[0][1]) and torch.equal(five[1][4], fw[0][2]) and
                                    torch.equal(five[1][1], st[0][0]) and torch.equal(five[1][4], st[0][1]))
                    burst, rounds = (8, 3) if nq <= 8 else ((2, 1) if nq <= 64 else (1, 1))
                    runs = {name: [] for name in calls}
                    for _ in range(3):
                        for name, fn in calls.items():
                            runs[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                    ctx.sync()
                    med = {name: statistics.median(v) for name, v in runs.items()}
                    if layout == "fixed":
                        bound = 1.0 + DECODE_VALU * (k - 1) / (STEP_VALU * READ_LEN)
                    else:
                        bound = SNAP_STEP_VALU / MASK_STEP_VALU + DECODE_VALU * (k - 1) / (MASK_STEP_VALU * longest)
                    bound += spread(runs["route"])
                    run = {"k": k, "n_queries": nq, "layout": layout, "form": form, "equals_oracle_on_sample": ok_sample, "full_rule_equals_route_on_all": ok_route,
                           "reads_with_an_adapter": found, "of_them_overhangs": overhangs,
                           "adapter_ms": round(med["adapter"], 4), "adapter_runs_ms": [round(x, 4) for x in runs["adapter"]], "adapter_spread": round(spread(runs["adapter"]), 4),
                           "route_ms": round(med["route"], 4), "route_runs_ms": [round(x, 4) for x in runs["route"]], "route_spread": round(spread(runs["route"]), 4),
                           "adapter_over_route": round(med["adapter"] / med["route"], 4), "bound": round(bound, 4)}
                    run["within_bound"] = run["adapter_over_route"] <= run["bound"]
                    total = n if layout == "fixed" else float(np.sum(b["off"][1:] - b["off"][:-1]))
                    run["adapter_ps_per_read_query_base"] = round(med["adapter"] * 1e9 / (total * nq), 4)
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
            del dq
    doc["all_equal"] = all(r["equals_oracle_on_sample"] and r["full_rule_equals_route_on_all"] for r in doc["runs"])
    doc["outside_bound_points"] = [{key: r[key] for key in ("k", "n_queries", "layout", "form", "adapter_over_route", "bound")} for r in doc["runs"] if not r["within_bound"]]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0 if doc["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
