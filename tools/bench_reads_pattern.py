"""The per-read matchers under pattern queries (bitnuc_reads_pattern_*_async) against their exact twins (bitnuc_reads_hdist_*_async) on the same data, in
one process.  The tile loops of a twin are the same code; only the kernels that build the per-query tables read 16 instead of 8 bytes per query, so the
expectation is a ratio of 1.0.

6,666,667 reads x 150 bases of the nucgen stream (seed 0xB17C0DE), encoded with encode_fixed_dev (5 words per read); k in {16, 31}; Q in {1, 8, 64, 512}
queries, half of them windows of reads at an admissible offset and half random.  Families: anchored (four offsets at the 3' end, all six outputs), best,
best2, and on the same reads under an offsets table anchored_batch (END, 0 .. 3) and best_batch; ASCII bytes and packed words.  Per point, three
alternating queues of
  exact        the exact twin on the 2-bit queries
  pattern      the pattern form on the singleton patterns of the same queries (equal outputs, checked on all reads)
  degenerate   the pattern form on a degenerate list of the same length: barcode + NNNN + linker (the middle four positions of every pattern are N)
timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported: the medians, the exact twin's own spread
over its three queues ((max - min) / median) -- the margin the ratios get --, pattern / exact and degenerate / exact, and whether each ratio lies within
that spread of 1.0.

    python tools/bench_reads_pattern.py [--out FILE] [--ks 16,31] [--qs 1,8,64,512] [--families anchored,best,...] [--forms ascii,packed] [--count N]
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
FAMILIES = ("anchored", "best", "best2", "anchored_batch", "best_batch")
NOFF = 4


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--forms", default="ascii,packed")
    ap.add_argument("--count", type=int, default=6_666_667)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import pattern_oracle as po
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    count, wpr = args.count, (READ_LEN + 31) // 32
    n = count * READ_LEN
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(count * wpr, dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, words)
    offsets = torch.arange(count + 1, dtype=torch.int64, device=dev) * READ_LEN
    word_offsets = torch.arange(count + 1, dtype=torch.int64, device=dev) * wpr
    ctx.sync()
    rng = np.random.default_rng(2031)
    doc = {"reads": count, "read_len": READ_LEN, "seed": SEED, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "offsets": NOFF, "runs": []}
    types = (torch.int32, torch.int32, torch.uint8)
    out = {kind: [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)] for kind in ("exact", "pattern")}
    pos_lo = lambda k: READ_LEN - k - (NOFF - 1)

    def call(kind, family, form, k, dq, nq, six):
        """the _async call of one (kind, family, form) into the output set `six`"""
        name = ("reads_hdist_" if kind == "exact" else "reads_pattern_") + family + ("_packed" if form == "packed" else "") + "_async"
        fn = getattr(ctx, name)
        src = ref if form == "ascii" else words
        if family == "anchored":
            return fn(src, READ_LEN, count, k, dq, nq, *six, pos_lo=pos_lo(k), pos_hi=None)
        if family == "best":
            return fn(src, READ_LEN, count, k, dq, nq, *six[:3])
        if family == "best2":
            return fn(src, READ_LEN, count, k, dq, nq, *six)
        tabs = (offsets, count, n) if form == "ascii" else (word_offsets, offsets, count, count * wpr)
        if family == "anchored_batch":
            return fn(src, *tabs, k, dq, nq, *six, pos_lo=0, pos_hi=NOFF - 1, anchor="end")
        return fn(src, *tabs, k, dq, nq, *six[:3])

    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            qs = []
            for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, NOFF, size=(nq + 1) // 2)):
                at = int(r) * READ_LEN + pos_lo(k) + int(p)
                h = ref[at:at + k].cpu().numpy()
                qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            single = np.stack([po.from_2bit(q, k) for q in queries]).astype(np.uint32)
            mid = np.uint32(0xF << (k // 2 - 2))  # barcode + NNNN + linker: four N positions in the middle
            dq = {"exact": torch.from_numpy(queries.view(np.int64)).to(dev), "pattern": torch.from_numpy(single.view(np.int32)).to(dev),
                  "degenerate": torch.from_numpy((single | mid).view(np.int32)).to(dev)}
            for family in args.families.split(","):
                for form in args.forms.split(","):
                    nout = 3 if family in ("best", "best_batch") else 6
                    fns = {"exact": lambda i: call("exact", family, form, k, dq["exact"], nq, out["exact"][i & 1]),
                           "pattern": lambda i: call("pattern", family, form, k, dq["pattern"], nq, out["pattern"][i & 1]),
                           "degenerate": lambda i: call("pattern", family, form, k, dq["degenerate"], nq, out["pattern"][i & 1])}
                    for a in out["exact"][0] + out["pattern"][0]:
                        a.fill_(0x5A)
                    fns["exact"](0)
                    fns["pattern"](0)
                    ctx.sync()
                    equal = all(bool(torch.equal(a, b)) for a, b in zip(out["exact"][0][:nout], out["pattern"][0][:nout]))
                    whole = family in ("best", "best2", "best_batch")
                    burst, rounds = ((8, 3) if nq <= 64 else (4, 2)) if not whole else ((4, 2) if nq <= 8 else (2, 1))
                    runs = {name: [] for name in fns}
                    for _ in range(3):  # alternating queues
                        for name, fn in fns.items():
                            runs[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                    ctx.sync()
                    med = {name: statistics.median(v) for name, v in runs.items()}
                    margin = spread(runs["exact"])
                    run = {"k": k, "n_queries": nq, "family": family, "form": form, "equal_to_exact_twin": equal,
                           "exact_ms": round(med["exact"], 4), "exact_runs_ms": [round(x, 4) for x in runs["exact"]], "exact_spread": round(margin, 4),
                           "pattern_ms": round(med["pattern"], 4), "pattern_runs_ms": [round(x, 4) for x in runs["pattern"]],
                           "degenerate_ms": round(med["degenerate"], 4), "degenerate_runs_ms": [round(x, 4) for x in runs["degenerate"]],
                           "pattern_over_exact": round(med["pattern"] / med["exact"], 4), "degenerate_over_exact": round(med["degenerate"] / med["exact"], 4),
                           "pattern_within_spread": bool(abs(med["pattern"] / med["exact"] - 1.0) <= margin),
                           "degenerate_within_spread": bool(abs(med["degenerate"] / med["exact"] - 1.0) <= margin)}
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
    doc["all_equal"] = all(r["equal_to_exact_twin"] for r in doc["runs"])
    doc["all_within_spread"] = all(r["pattern_within_spread"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
