"""The best match and the runner-up per read (bitnuc_reads_hdist_best2[_packed]_async, scan_reads_device.h's exclusion form) against the best match
per read alone (bitnuc_reads_hdist_best[_packed]_async) on the same data.  The yardstick is 2.0: best2 is two passes of the best match's kernels (none
of the second with one query) and one kernel that writes six outputs instead of three.  One process.

6,666,667 reads x 150 bases of the nucgen stream (seed 0xB17C0DE), encoded with encode_fixed_dev (5 words per read); k = 31; Q in {1, 8, 64, 512}
queries, half of them windows of reads and half random.  For each Q and input form (ASCII bytes, packed words): best2 and best in alternating queues,
three of each, timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported per point: the ratio
best2 / best of the medians and each call's own spread over its three queues ((max - min) / median).  The six arrays of best2 are compared with
tests/reads_best2_oracle.py on the first --sample reads, and its first three with best's on all reads (both must be equal).

    python tools/bench_reads_best2.py [--out FILE] [--k 31] [--qs 1,8,64,512] [--count 6666667] [--sample 256]      one JSON document
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=256)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_best2_oracle as r2
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    count, k, wpr = args.count, args.k, (READ_LEN + 31) // 32
    n = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(count * wpr, dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, words)
    ctx.sync()
    head = ref[:sample * READ_LEN].cpu().numpy()
    rng = np.random.default_rng(2029)
    doc = {"reads": count, "read_len": READ_LEN, "k": k, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0),
           "library": L.load().bitnuc_version().decode(), "runs": []}
    nw = READ_LEN - k + 1
    types = (torch.int32, torch.int32, torch.uint8)
    for nq in [int(x) for x in args.qs.split(",")]:
        qs = []
        for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, nw, size=(nq + 1) // 2)):
            at = int(r) * READ_LEN + int(p)
            h = ref[at:at + k].cpu().numpy()
            qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
        qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
        queries = np.array(qs, dtype=np.uint64)
        dq = torch.from_numpy(queries.view(np.int64)).to(dev)
        six = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
        three = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types) for _ in range(2)]
        want = r2.reads_best2(head, READ_LEN, sample, k, queries)
        forms = {
            "ascii": (lambda i: ctx.reads_hdist_best2_async(ref, READ_LEN, count, k, dq, nq, *six[i & 1]),
                      lambda i: ctx.reads_hdist_best_async(ref, READ_LEN, count, k, dq, nq, *three[i & 1])),
            "packed": (lambda i: ctx.reads_hdist_best2_packed_async(words, READ_LEN, count, k, dq, nq, *six[i & 1]),
                       lambda i: ctx.reads_hdist_best_packed_async(words, READ_LEN, count, k, dq, nq, *three[i & 1])),
        }
        for form, (best2, best) in forms.items():
            for a in six[0] + three[0]:
                a.fill_(0x5A)
            best2(0)
            best(0)
            ctx.sync()
            got = [a[:sample].cpu().numpy() for a in six[0]]
            equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
            equal_best = all(bool(torch.equal(a, b)) for a, b in zip(six[0][:3], three[0]))
            burst, rounds = (8, 5) if nq <= 8 else ((4, 3) if nq <= 64 else (2, 2))
            a_runs, b_runs = [], []
            for _ in range(3):  # alternating queues
                a_runs.append(timed_sustained(torch, stream, best2, burst=burst, rounds=rounds))
                b_runs.append(timed_sustained(torch, stream, best, burst=burst, rounds=rounds))
            ctx.sync()
            a_ms, b_ms = statistics.median(a_runs), statistics.median(b_runs)
            run = {"n_queries": nq, "form": form, "equal_to_oracle_on_sample": equal_oracle, "best_triple_equal_to_best": equal_best,
                   "best2_burst_ms": round(a_ms, 4), "best2_runs_ms": [round(x, 4) for x in a_runs],
                   "best2_spread": round((max(a_runs) - min(a_runs)) / a_ms, 4),
                   "best_burst_ms": round(b_ms, 4), "best_runs_ms": [round(x, 4) for x in b_runs],
                   "best_spread": round((max(b_runs) - min(b_runs)) / b_ms, 4),
                   "best2_over_best": round(a_ms / b_ms, 4),
                   "ambiguous_reads": int(((six[0][5] - six[0][2]) < 2).sum()) if nq > 1 else 0}
            doc["runs"].append(run)
            print(json.dumps(run), flush=True)
        del dq, six, three
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["best_triple_equal_to_best"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
