"""The indel-tolerant family's second stage -- where the alignment that ends at a given base starts (bitnuc_reads_edist_start*_async,
bitnuc_ref_edist_start*_async; edist_start_kernel) -- against a yardstick of the same shape and next to the forward calls it follows.  One process.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE) as two batches of --count reads: every read 150 bases (fixed layout) and lengths uniform in
[100, 200] (ragged layout; the last read takes up the rest).  k in {16, 31}; ASCII bytes and packed words.  Three alternating queues of each form per point,
timed as bench.py times its config-5 block (timed_sustained).
  1. start / yardstick.  The yardstick is bitnuc_reads_edist_anchored*_async with ONE query and pos_hi - pos_lo = k - 1 on the same reads in the same
     queues: span 2k - 1, the same number of steps per read, about the same bytes read and validated.  The start call runs on the yardstick's own
     (best_query, best_end) with the floor at pos_lo ("mixed": w = end - pos_lo differs from lane to lane, the masked loop) and on ends at
     pos_lo + 2k - 1 ("full": every lane walks 2k - 1 bases, the unmasked loop).  Held against 1 + 1.25 / 20 (the masked loop; "full": 1) + STEP_EXTRA / 20 (4.75 masked, 4 full)
     + ITEM_VALU / (20 (2k - 1)) + the yardstick's own spread, with STEP_EXTRA and ITEM_VALU from the shipped disassembly.
  2. the price of the start: (forward + start) / forward at Q in {1, 8, 64, 512} for the whole-read form and the anchored form.
  3. along --n reference bases: (hits + start) / hits at the sparse points of tools/bench_kmer_edist_hits.py (tau in {0, 2}, cap 2^20), the start call fed
     by the hit list's device count.
Every start output is compared with tests/edist_start_oracle.py on the first --sample items, and dist with the forward call's on all items.

    python tools/bench_edist_start.py [--out FILE] [--ks 16,31] [--qs 1,8,64,512] [--count 6666667] [--n 1000000000] [--sample 64]   one JSON document
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
STEP_VALU = 20.0   # the yardstick's vector instructions per (read, query, base), four queries side by side
MASK_VALU = 1.25   # what a masked loop adds per (query, step)
STEP_EXTRA = {True: 4.75, False: 4.0}  # by masked: the shipped loops have 26 / 24 vector instructions a step against the yardstick's 21.25 / 20 per query -- the
#                    extraction of the code bits and the loop's compare are not shared by four queries, the carry-in is an or of its own, the mask a compare and a select
ITEM_VALU = 40.0   # per item, an estimate from the disassembly: the table entry's load, four bit reversals and shifts, the 128-bit shift of the window


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
    ap.add_argument("--n", type=int, default=1_000_000_000)
    ap.add_argument("--sample", type=int, default=64)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import edist_start_oracle as so
    import reads_best_oracle as ro
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)
    count = args.count
    n = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(max(n, args.n), dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, ref.numel(), SEED)
    ctx.sync()
    rng = np.random.default_rng(2431)
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
    doc = {"reads": count, "bases": n, "seed": SEED, "sample_items": sample, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "ragged_lengths": [100, 200], "yardstick": "bitnuc_reads_edist_anchored*_async, one query, pos_hi - pos_lo = k - 1 (span 2k - 1)",
           "step_valu_yardstick": STEP_VALU, "masked_loop_adds": MASK_VALU, "step_extra_valu": {"masked": STEP_EXTRA[True], "full": STEP_EXTRA[False]}, "item_valu": ITEM_VALU, "yardstick_runs": [],
           "price_runs": [], "reference_runs": []}
    i32, u8 = torch.int32, torch.uint8
    fw = [tuple(torch.zeros(count, dtype=t, device=dev) for t in (i32, i32, u8)) for _ in range(2)]
    st = [(torch.zeros(count, dtype=i32, device=dev), torch.zeros(count, dtype=u8, device=dev)) for _ in range(2)]

    def oracle_ok(b, k, anchor_end, pos, queries, fq, fe, got):
        codes = ro.codes_of(b["head"])
        off = [int(x) for x in b["off"][:sample + 1]]
        texts = [codes[off[r]:off[r + 1]] for r in range(sample)]
        floors = [so.floor_of(len(t), k, anchor_end, pos) for t in texts]
        ws, wd = so.starts(texts, floors, so.masks_of(queries, k), k, fq[:sample], fe[:sample])
        return bool(np.array_equal(got[0][:sample], ws.astype(np.uint32)) and np.array_equal(got[1][:sample], wd))

    for k in [int(x) for x in args.ks.split(",")]:
        pos_lo = READ_LEN - (2 * k - 1)  # the 3' end: the span is the read's last 2k - 1 bases
        at = int(rag["off"][12345]) + 60
        queries = np.array([word_of(ref[at:at + k].cpu().numpy())], dtype=np.uint64)
        dq = torch.from_numpy(queries.view(np.int64)).to(dev)
        full_end = torch.full((count,), pos_lo + 2 * k - 1, dtype=i32, device=dev)
        zero_q = torch.zeros(count, dtype=i32, device=dev)
        for form in ("ascii", "packed"):
            pk = "" if form == "ascii" else "_packed"
            src = ref if form == "ascii" else equal["words"]
            bhead = (ref, rag["d_off"], count, n) if form == "ascii" else (rag["words"], rag["d_wtab"], rag["d_off"], count, int(rag["wtab"][-1]))
            yard, yard_b = getattr(ctx, "reads_edist_anchored" + pk + "_async"), getattr(ctx, "reads_edist_anchored_batch" + pk + "_async")
            start, start_b = getattr(ctx, "reads_edist_start" + pk + "_async"), getattr(ctx, "reads_edist_start_batch" + pk + "_async")
            yq, ye, yd = (torch.zeros(count, dtype=t, device=dev) for t in (i32, i32, u8))
            bq, be, bd = (torch.zeros(count, dtype=t, device=dev) for t in (i32, i32, u8))
            yard(src, READ_LEN, count, k, dq, 1, yq, ye, yd, pos_lo=pos_lo, pos_hi=pos_lo + k - 1)
            yard_b(*bhead, k, dq, 1, bq, be, bd, pos_lo=0, pos_hi=k - 1, anchor="end")
            ctx.sync()
            calls = {
                "yardstick": lambda i: yard(src, READ_LEN, count, k, dq, 1, *fw[i & 1], pos_lo=pos_lo, pos_hi=pos_lo + k - 1),
                "start_mixed": lambda i: start(src, READ_LEN, count, k, dq, 1, yq, ye, *st[i & 1], "start", pos_lo),
                "start_full": lambda i: start(src, READ_LEN, count, k, dq, 1, zero_q, full_end, *st[i & 1], "start", pos_lo),
                "yardstick_ragged": lambda i: yard_b(*bhead, k, dq, 1, *fw[i & 1], pos_lo=0, pos_hi=k - 1, anchor="end"),
                "start_ragged": lambda i: start_b(*bhead, k, dq, 1, bq, be, *st[i & 1], "end", k - 1),
            }
            checks = {}
            for name, fq_, fe_, fd_, b, floor in (("start_mixed", yq, ye, yd, equal, (0, pos_lo)), ("start_ragged", bq, be, bd, rag, (1, k - 1))):
                calls[name](0)
                ctx.sync()
                got = (st[0][0].cpu().numpy().view(np.uint32), st[0][1].cpu().numpy())
                checks[name + "_equals_oracle_on_sample"] = oracle_ok(b, k, floor[0], floor[1], queries, fq_.cpu().numpy().view(np.uint32), fe_.cpu().numpy().view(np.uint32), got)
                checks[name + "_dist_equals_forward_on_all"] = bool(torch.equal(st[0][1], fd_))
            runs = {name: [] for name in calls}
            for _ in range(3):
                for name, fn in calls.items():
                    runs[name].append(timed_sustained(torch, stream, fn, burst=8, rounds=3))
            ctx.sync()
            med = {name: statistics.median(v) for name, v in runs.items()}
            run = {"k": k, "form": form, **checks}
            for name in calls:
                run[name + "_ms"] = round(med[name], 4)
                run[name + "_runs_ms"] = [round(x, 4) for x in runs[name]]
                run[name + "_spread"] = round(spread(runs[name]), 4)
            per_item = ITEM_VALU / (STEP_VALU * (2 * k - 1))
            for name, yname, masked in (("start_mixed", "yardstick", True), ("start_full", "yardstick", False), ("start_ragged", "yardstick_ragged", True)):
                run[name + "_over_yardstick"] = round(med[name] / med[yname], 4)
                run[name + "_bound"] = round(1.0 + (MASK_VALU / STEP_VALU if masked else 0.0) + STEP_EXTRA[masked] / STEP_VALU + per_item + spread(runs[yname]), 4)
                run[name + "_within_bound"] = run[name + "_over_yardstick"] <= run[name + "_bound"]
            doc["yardstick_runs"].append(run)
            print(json.dumps(run), flush=True)
            # the price of the start behind the whole-read form and the anchored form
            best = getattr(ctx, "reads_edist_best" + pk + "_async")
            for nq in [int(x) for x in args.qs.split(",")]:
                qs = [word_of(ref[int(a):int(a) + k].cpu().numpy()) for a in rng.integers(0, n - k, size=(nq + 1) // 2)] + [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
                dqs = torch.from_numpy(np.array(qs, dtype=np.uint64).view(np.int64)).to(dev)
                span_hi = pos_lo + k - 1
                pcalls = {
                    "best": lambda i: best(src, READ_LEN, count, k, dqs, nq, *fw[i & 1]),
                    "best_start": lambda i: (best(src, READ_LEN, count, k, dqs, nq, *fw[i & 1]),
                                             start(src, READ_LEN, count, k, dqs, nq, fw[i & 1][0], fw[i & 1][1], *st[i & 1], "start", 0)),
                    "anchored": lambda i: yard(src, READ_LEN, count, k, dqs, nq, *fw[i & 1], pos_lo=pos_lo, pos_hi=span_hi),
                    "anchored_start": lambda i: (yard(src, READ_LEN, count, k, dqs, nq, *fw[i & 1], pos_lo=pos_lo, pos_hi=span_hi),
                                                 start(src, READ_LEN, count, k, dqs, nq, fw[i & 1][0], fw[i & 1][1], *st[i & 1], "start", pos_lo)),
                }
                pcalls["best_start"](0)
                ctx.sync()
                dist_ok = bool(torch.equal(st[0][1], fw[0][2]))
                burst, rounds = (8, 3) if nq <= 8 else ((2, 1) if nq <= 64 else (1, 1))
                pruns = {name: [] for name in pcalls}
                for _ in range(3):
                    for name, fn in pcalls.items():
                        pruns[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                ctx.sync()
                pm = {name: statistics.median(v) for name, v in pruns.items()}
                prun = {"k": k, "form": form, "n_queries": nq, "dist_equals_forward_on_all": dist_ok}
                for name in pcalls:
                    prun[name + "_ms"] = round(pm[name], 4)
                    prun[name + "_spread"] = round(spread(pruns[name]), 4)
                prun["best_with_start_over_best"] = round(pm["best_start"] / pm["best"], 4)
                prun["anchored_with_start_over_anchored"] = round(pm["anchored_start"] / pm["anchored"], 4)
                doc["price_runs"].append(prun)
                print(json.dumps(prun), flush=True)
                del dqs
    # along a reference: the hit list and the start call it feeds through its device count
    nref = args.n
    words = torch.zeros((nref + 31) // 32, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref[:nref], nref, words)
    ctx.sync()
    cap = 1 << 20
    d_end = [torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(2)]
    d_hd = [torch.zeros(cap, dtype=u8, device=dev) for _ in range(2)]
    d_n = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2)]
    d_st = [torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(2)]
    d_sd = [torch.zeros(cap, dtype=u8, device=dev) for _ in range(2)]
    for k in [int(x) for x in args.ks.split(",")]:
        at = nref // 3
        query = word_of(ref[at:at + k].cpu().numpy())
        dq = torch.from_numpy(np.array([query], dtype=np.uint64).view(np.int64)).to(dev)
        for form in ("ascii", "packed"):
            head = (ref, nref) if form == "ascii" else (words, words.numel(), nref)
            pk = "" if form == "ascii" else "_packed"
            hits, startf = getattr(ctx, "kmer_edist_hits" + pk + "_async"), getattr(ctx, "kmer_edist_start" + pk + "_async")
            for tau in (0, 2):
                rcalls = {
                    "hits": lambda i: hits(*head, k, query, tau, d_end[i & 1], d_hd[i & 1], cap, d_n[i & 1]),
                    "hits_start": lambda i: (hits(*head, k, query, tau, d_end[i & 1], d_hd[i & 1], cap, d_n[i & 1]),
                                             startf(*head, k, dq, 1, None, d_end[i & 1], cap, d_st[i & 1], d_sd[i & 1], d_m=d_n[i & 1])),
                }
                rcalls["hits_start"](0)
                ctx.sync()
                total = int(d_n[0].item())
                m = min(total, cap)
                ok = bool(torch.equal(d_sd[0][:m], d_hd[0][:m])) and bool((d_st[0][:m] <= d_end[0][:m]).all())
                rruns = {name: [] for name in rcalls}
                for _ in range(3):
                    for name, fn in rcalls.items():
                        rruns[name].append(timed_sustained(torch, stream, fn, burst=4, rounds=2))
                ctx.sync()
                rm = {name: statistics.median(v) for name, v in rruns.items()}
                rrun = {"k": k, "form": form, "tau": tau, "n_hits": total, "dist_equals_hit_dist_and_start_le_end": ok, "hits_ms": round(rm["hits"], 4),
                        "hits_spread": round(spread(rruns["hits"]), 4), "hits_start_ms": round(rm["hits_start"], 4),
                        "hits_with_start_over_hits": round(rm["hits_start"] / rm["hits"], 4)}
                doc["reference_runs"].append(rrun)
                print(json.dumps(rrun), flush=True)
    doc["all_equal"] = all(all(v for key, v in r.items() if key.endswith(("_on_sample", "_on_all"))) for r in doc["yardstick_runs"] + doc["price_runs"]) and \
        all(r["dist_equals_hit_dist_and_start_le_end"] for r in doc["reference_runs"])
    doc["outside_bound_points"] = [{"k": r["k"], "form": r["form"], "what": name, "ratio": r[name + "_over_yardstick"], "bound": r[name + "_bound"]}
                                   for r in doc["yardstick_runs"] for name in ("start_mixed", "start_full", "start_ragged") if not r[name + "_within_bound"]]
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
