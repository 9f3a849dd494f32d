"""The indel-tolerant hit list (bitnuc_kmer_edist_hits[_packed]_async and the pattern twins, scan_edist_hits_device.h) next to the edit-distance count
on the same query and tau (the hit list's count pass is that walk: the ratio shows what the scan and the emit pass add), next to the Hamming hit list
on the same arguments (ANOTHER ANSWER: the ratio is the price of indel tolerance) and next to its own pattern twin.  One process.

--n bases (default 10^9) of the nucgen stream (seed 0xB17C0DE), as ASCII bytes and as packed words; k in {16, 23, 31}; the query is a window of the
reference.  Per (k, form):
  sparse   tau in {0, 2}, cap 2^20: three alternating queues of  hits  (the exact form),  count  (bitnuc_kmer_edist_count_multi*_async, Q = 1),
           hdist_hits  (bitnuc_kmer_hdist_hits*_dev)  and  pattern  (the twin on the query's singleton pattern); the medians, each form's own spread
           ((max - min) / median), hits / count, hits / hdist_hits, pattern / hits, the number of hits and the share of non-empty chunks and waves
           (from the list itself: an end j lies in chunk (j - 1) / 1024, 64 chunks to a wave);
  dense    tau = k, cap = n (9 bytes written per end): hits and hdist_hits, three alternating queues, the write rate 9 n / t.
Timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  The outputs are compared with
tests/kmer_edist_oracle.py on the first --sample bases (a call of its own on that prefix), *n_hits with the count on the whole reference, the pattern
twin's list with the exact form's.

    python tools/bench_kmer_edist_hits.py [--out FILE] [--n 1000000000] [--ks 16,23,31] [--sample 200000] [--no-dense]      one JSON document
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
CHUNK = 1024
CAP = 1 << 20


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--ks", default="16,23,31")
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--no-dense", action="store_true")
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import kmer_edist_hits_oracle as ho
    import pattern_oracle as po
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    n = args.n
    nw = (n + 31) // 32
    sample = min(args.sample, n)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, n, words)
    ctx.sync()
    head_codes = po.codes_of_ascii(ref[:sample].cpu().numpy())
    rng = np.random.default_rng(2033)
    doc = {"bases": n, "seed": SEED, "sample_bases": sample, "cap_sparse": CAP, "device": torch.cuda.get_device_name(0),
           "library": L.load().bitnuc_version().decode(), "runs": []}
    cap_dense = 0 if args.no_dense else n
    ends = [torch.zeros(max(CAP, cap_dense), dtype=torch.int64, device=dev) for _ in range(2)]
    dists = [torch.zeros(max(CAP, cap_dense), dtype=torch.uint8, device=dev) for _ in range(2)]
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    for k in [int(x) for x in args.ks.split(",")]:
        at = int(rng.integers(sample // 2, sample - k))  # a window of the prefix: the oracle sees at least one hit
        h = ref[at:at + k].cpu().numpy()
        q = int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h)))
        sing = po.from_2bit(q, k)
        dq = torch.from_numpy(np.array([q], dtype=np.uint64).view(np.int64)).to(dev)
        for form in ("ascii", "packed"):
            src = (ref, n) if form == "ascii" else (words, nw, n)
            small = (ref, sample) if form == "ascii" else (words, (sample + 31) // 32, sample)
            sfx = "" if form == "ascii" else "_packed"
            fe, fp = (getattr(ctx, f"kmer_{x}edist_hits{sfx}_async") for x in ("", "pattern_"))
            fc = getattr(ctx, f"kmer_edist_count_multi{sfx}_async")
            fh = getattr(ctx, f"kmer_hdist_hits{sfx}_dev")
            for tau in (0, 2) + (() if args.no_dense else (k,)):
                dense = tau == k
                cap = cap_dense if dense else CAP
                dt = torch.full((1,), tau, dtype=torch.int32, device=dev)
                hits = lambda i, a=src, c=cap: fe(*a, k, q, tau, ends[i & 1], dists[i & 1], c, totals[i & 1:])
                pattern = lambda i: fp(*src, k, sing, tau, ends[i & 1], dists[i & 1], cap, totals[2 + (i & 1):])
                count = lambda i: fc(*src, k, dq, dt, 1, counts[i & 1:])
                hdist = lambda i: fh(*src, k, q, tau, ends[i & 1], dists[i & 1], cap, totals[2 + (i & 1):])
                # the prefix against the oracle
                want = ho.hits(head_codes, k, sing, tau)
                hits(0, small, min(cap, CAP))
                ctx.sync()
                m = min(int(totals[0]), min(cap, CAP))
                equal_oracle = bool(int(totals[0]) == want[0].size and np.array_equal(ends[0][:m].cpu().numpy().view(np.uint64), want[0][:m]) and
                                    np.array_equal(dists[0][:m].cpu().numpy(), want[1][:m]))
                # the whole reference: the count, the pattern twin
                hits(0)
                count(0)
                ctx.sync()
                total = int(totals[0])
                m = min(total, cap)
                equal_count = bool(total == int(counts[0]))
                e0 = ends[0][:m].clone()
                d0 = dists[0][:m].clone()
                pattern(1)
                ctx.sync()
                equal_pattern = bool(int(totals[3]) == total and torch.equal(ends[1][:m], e0) and torch.equal(dists[1][:m], d0))
                ascending = bool(m < 2 or (e0[1:] > e0[:-1]).all())
                if dense:  # every end a hit: every chunk
                    nonempty_chunks, nonempty_waves = (n + CHUNK - 1) // CHUNK, (n + 64 * CHUNK - 1) // (64 * CHUNK)
                else:
                    chunks = torch.unique((e0 - 1) // CHUNK)
                    nonempty_chunks = int(chunks.numel())
                    nonempty_waves = int(torch.unique(chunks // 64).numel())
                    del chunks
                del e0, d0
                hdist(0)
                ctx.sync()
                hdist_total = int(totals[2])
                forms = {"hits": hits, "hdist_hits": hdist} if dense else {"hits": hits, "count": count, "hdist_hits": hdist, "pattern": pattern}
                burst, rounds = (1, 1) if dense else (2, 2)
                runs = {name: [] for name in forms}
                for _ in range(3):  # alternating queues
                    for name, fn in forms.items():
                        runs[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                ctx.sync()
                med = {name: statistics.median(v) for name, v in runs.items()}
                nch = (n + CHUNK - 1) // CHUNK
                run = {"k": k, "form": form, "tau": tau, "case": "dense" if dense else "sparse", "cap": cap, "n_hits": total, "hdist_n_hits": hdist_total,
                       "nonempty_chunks": nonempty_chunks, "chunks": nch, "nonempty_waves": nonempty_waves, "waves": (nch + 63) // 64,
                       "equal_to_oracle_on_sample": equal_oracle, "n_hits_equal_to_count": equal_count, "pattern_equal_to_exact": equal_pattern,
                       "ascending": ascending}
                for name in forms:
                    run[name + "_ms"] = round(med[name], 4)
                    run[name + "_runs_ms"] = [round(x, 4) for x in runs[name]]
                    run[name + "_spread"] = round(spread(runs[name]), 4)
                run["hits_over_hdist_hits"] = round(med["hits"] / med["hdist_hits"], 3)
                if dense:
                    run["write_gb_per_s"] = round(9.0 * m / med["hits"] / 1e6, 1)
                    run["hdist_write_gb_per_s"] = round(9.0 * min(hdist_total, cap) / med["hdist_hits"] / 1e6, 1)
                else:
                    run["hits_over_count"] = round(med["hits"] / med["count"], 4)
                    run["pattern_over_hits"] = round(med["pattern"] / med["hits"], 4)
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["n_hits_equal_to_count"] and r["pattern_equal_to_exact"] and r["ascending"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
