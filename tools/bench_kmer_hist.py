"""The mismatch histogram per query (bitnuc_kmer_hdist_hist[_packed]_async and the pattern twins, scan_hist_device.h) against the two things it stands
between, in one process:
  (a) the multi-query count with every query repeated n_bins times at thresholds 0 .. n_bins - 1 -- the route the header recommended for a mismatch
      profile before this call existed; its prefix differences must equal the histogram (checked here);
  (b) the best match at the same Q -- the same four-channel contraction with the cheapest back end there is; the first non-zero bin must be its
      distance where that is below n_bins (checked here).

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device.  k = 31: exact queries, half of them windows of the sequence with 0 .. 3 bases
changed and half random; k = 23: patterns, a guide of twenty bases taken from the sequence (0 .. 3 changed) + NGG.  Q in {1, 8, 64, 512}, n_bins in
{4, 8, 16}, ASCII bytes and packed words.  Per form three queues of back-to-back launches, ALTERNATING between the three forms (hist, a, b, hist, a,
b, ...) so that a drift of the chip's clock meets all three alike; a form's figure is the median of its three queues and its spread (max - min) /
median.  A ratio closer to 1 than the two forms' spreads together is reported as no difference.

    python tools/bench_kmer_hist.py [--out profiles/r12_kmer_hist.json] [--ks 31,23] [--qs 1,8,64,512] [--bins 4,8,16]      one JSON document
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0xB17C0DE
N = 10**9
QUEUES = 3


def queue_ms(torch, stream, fn, burst):
    """ms per launch of `burst` back-to-back launches behind one warm-up launch of the same form"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    a.record(stream)
    for i in range(burst):
        fn(1 + i)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def pattern_of(codes20):
    """twenty exact positions + N + G + G -> (4,) uint32"""
    p = np.zeros(4, dtype=np.uint32)
    for i, c in enumerate(codes20):
        p[int(c)] |= np.uint32(1 << i)
    for c in range(4):
        p[c] |= np.uint32(1 << 20)
    p[2] |= np.uint32((1 << 21) | (1 << 22))
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="31,23")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--bins", default="4,8,16")
    ap.add_argument("--n", type=int, default=N)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    n = args.n
    nw = (n + 31) // 32
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, n, words)
    ctx.sync()
    rng = np.random.default_rng(2031)
    doc = {"n_bases": n, "seed": SEED, "queues_per_form": QUEUES, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(),
           "runs": []}
    for k in [int(x) for x in args.ks.split(",")]:
        pattern = k == 23
        for nq in [int(x) for x in args.qs.split(",")]:
            rows = []
            for i in range(nq):
                if pattern or i % 2 == 0:
                    p = int(rng.integers(0, n - k))
                    h = ref[p:p + k].cpu().numpy()
                    c = (((h >> 1) ^ (h >> 2)) & 3).astype(np.int64)
                    at = rng.choice(20, size=int(rng.integers(0, 4)), replace=False)
                    c[at] = (c[at] + 1) & 3
                else:
                    c = rng.integers(0, 4, size=k)
                rows.append(pattern_of(c[:20]) if pattern else np.uint64(sum(int(x) << (2 * b) for b, x in enumerate(c))))
            if pattern:
                q = torch.from_numpy(np.stack(rows).view(np.int32)).to(dev)
            else:
                q = torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).to(dev)
            bp = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            bd = torch.zeros((2, nq), dtype=torch.uint8, device=dev)
            for n_bins in [int(x) for x in args.bins.split(",")]:
                rq = q.repeat_interleave(n_bins, dim=0).contiguous()  # (a): query i at thresholds 0 .. n_bins - 1
                rt = torch.arange(n_bins, dtype=torch.int32, device=dev).repeat(nq).contiguous()
                hist = torch.zeros((2, nq, n_bins), dtype=torch.int64, device=dev)
                cm = torch.zeros((2, nq * n_bins), dtype=torch.int64, device=dev)
                if pattern:
                    forms = {
                        "ascii": (lambda i: ctx.kmer_pattern_hist_async(ref, n, k, q, nq, n_bins, hist[i & 1]),
                                  lambda i: ctx.kmer_pattern_count_multi_async(ref, n, k, rq, rt, nq * n_bins, cm[i & 1]),
                                  lambda i: ctx.kmer_pattern_best_async(ref, n, k, q, nq, bp[i & 1], bd[i & 1])),
                        "packed": (lambda i: ctx.kmer_pattern_hist_packed_async(words, nw, n, k, q, nq, n_bins, hist[i & 1]),
                                   lambda i: ctx.kmer_pattern_count_multi_packed_async(words, nw, n, k, rq, rt, nq * n_bins, cm[i & 1]),
                                   lambda i: ctx.kmer_pattern_best_packed_async(words, nw, n, k, q, nq, bp[i & 1], bd[i & 1])),
                    }
                else:
                    forms = {
                        "ascii": (lambda i: ctx.kmer_hdist_hist_async(ref, n, k, q, nq, n_bins, hist[i & 1]),
                                  lambda i: ctx.kmer_hdist_count_multi_dev(ref, n, k, rq, rt, nq * n_bins, cm[i & 1]),
                                  lambda i: ctx.kmer_hdist_best_async(ref, n, k, q, nq, bp[i & 1], bd[i & 1])),
                        "packed": (lambda i: ctx.kmer_hdist_hist_packed_async(words, nw, n, k, q, nq, n_bins, hist[i & 1]),
                                   lambda i: ctx.kmer_hdist_count_multi_packed_dev(words, nw, n, k, rq, rt, nq * n_bins, cm[i & 1]),
                                   lambda i: ctx.kmer_hdist_best_packed_async(words, nw, n, k, q, nq, bp[i & 1], bd[i & 1])),
                    }
                for form, fns in forms.items():
                    for fn in fns:
                        fn(0)
                    ctx.sync()
                    h = hist[0].cpu().numpy()
                    c = cm[0].cpu().numpy().reshape(nq, n_bins)
                    prefix_equal = bool(np.array_equal(np.diff(c, axis=1, prepend=0), h))
                    d = bd[0].cpu().numpy()
                    first = np.where(h.any(axis=1), h.astype(bool).argmax(axis=1), 255)
                    best_equal = bool(np.array_equal(np.where(d < n_bins, d, 255), first))
                    burst = 4 if nq <= 8 else (2 if nq <= 64 else 1)
                    ms = [[], [], []]
                    for _ in range(QUEUES):  # alternating: hist, (a), (b), hist, (a), (b), ...
                        for j, fn in enumerate(fns):
                            ms[j].append(queue_ms(torch, stream, fn, burst))
                    med = [statistics.median(x) for x in ms]
                    spread = [(max(x) - min(x)) / statistics.median(x) for x in ms]
                    run = {"k": k, "kind": "pattern" if pattern else "exact", "n_queries": nq, "n_bins": n_bins, "form": form,
                           "prefix_differences_of_count_multi_equal_hist": prefix_equal, "first_nonzero_bin_equals_best": best_equal,
                           "hist_ms": round(med[0], 4), "count_multi_route_ms": round(med[1], 4), "best_ms": round(med[2], 4),
                           "hist_spread": round(spread[0], 4), "count_multi_route_spread": round(spread[1], 4), "best_spread": round(spread[2], 4),
                           "hist_over_count_multi_route": round(med[0] / med[1], 4), "hist_over_best": round(med[0] / med[2], 4),
                           "windows_in_bins": int(h.sum())}
                    run["faster_than_count_multi_route"] = ("yes" if med[0] / med[1] < 1 - (spread[0] + spread[1]) else
                                                            "no" if med[0] / med[1] > 1 + (spread[0] + spread[1]) else "no difference")
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
                del rq, rt, hist, cm
            del q, bp, bd
    doc["checks_hold_everywhere"] = all(r["prefix_differences_of_count_multi_equal_hist"] and r["first_nonzero_bin_equals_best"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
