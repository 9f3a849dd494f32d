"""The best match per query (bitnuc_kmer_hdist_best[_packed]_async, scan_best_device.h) against what the library offered before it -- Q calls of the
distance scan, each followed by an arg-min over its n-byte buffer -- and against the multi-query count as the structural yardstick, in one process
(DESIGN 3.4).

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device; k in {20, 31}; Q in {1, 8, 64, 512} queries, half of them windows of the
sequence (their best match is exact) and half random.  For each (k, Q) and input form (ASCII bytes, packed words):
  (a) the best-match call;
  (b) Q x (bitnuc_kmer_hdist_scan[_packed]_dev into a distance buffer + torch.argmin over it + a gather of the minimum);
  (c) bitnuc_kmer_hdist_count_multi[_packed]_dev with the same queries (thresholds cycling through 0, 3, 8, k);
timed as bench.py times its config-5 block: sustained bursts of back-to-back calls (timed_sustained) and, for (a), a short queue started on an idle
chip (timed_queue).  The positions and distances of (a) and (b) are compared (they must be equal).  Reported beside the times: (a) / (b), (a) / (c)
(four MFMAs per round against three: 4 / 3 where both are bound by the matrix pipe), the fraction of the matrix-pipe floor (Q x 4 MFMAs x 32 cycles
per 1024 windows over 1024 SIMDs at 2.4 GHz) and, at Q = 1, the single-query count's time.

    python tools/bench_kmer_best.py [--out FILE] [--ks 20,31] [--qs 1,8,64,512]      one JSON document
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import timed_queue, timed_sustained  # noqa: E402

SEED = 0xB17C0DE
N = 10**9
CLOCK_HZ, SIMDS = 2.4e9, 1024


def floor_ms(q, nwin):
    return q * 4 * 32 * (nwin / 1024) / SIMDS / CLOCK_HZ * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="20,31")
    ap.add_argument("--qs", default="1,8,64,512")
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    nw = (N + 31) // 32
    ref = torch.empty(N, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, N, SEED)
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, N, words)
    ctx.sync()
    dist = torch.empty((2, N), dtype=torch.uint8, device=dev)  # (b)'s distance bytes, alternating
    rng = np.random.default_rng(2027)
    doc = {"n_bases": N, "seed": SEED, "clock_hz_for_floor": CLOCK_HZ, "simds": SIMDS, "device": torch.cuda.get_device_name(0),
           "library": L.load().bitnuc_version().decode(), "runs": []}
    for k in [int(x) for x in args.ks.split(",")]:
        nwin = N - k + 1
        for nq in [int(x) for x in args.qs.split(",")]:
            qs = []
            for p in rng.integers(0, N - k, size=(nq + 1) // 2):
                h = ref[int(p):int(p) + k].cpu().numpy()
                qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            taus = np.array([(0, 3, 8, k)[i % 4] for i in range(nq)], dtype=np.uint32)
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            dt = torch.from_numpy(taus.view(np.int32)).to(dev)
            bp = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            bd = torch.zeros((2, nq), dtype=torch.uint8, device=dev)
            sp = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            sd = torch.zeros((2, nq), dtype=torch.uint8, device=dev)
            cm = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            one = torch.zeros(2, dtype=torch.int64, device=dev)

            def scans(i, scan):
                for j in range(nq):
                    d = dist[(i + j) & 1, :nwin]
                    scan(int(queries[j]), d)
                    at = torch.argmin(d)
                    sp[i & 1, j] = at
                    sd[i & 1, j] = d[at]

            forms = {
                "ascii": (lambda i: ctx.kmer_hdist_best_async(ref, N, k, dq, nq, bp[i & 1], bd[i & 1]),
                          lambda i: scans(i, lambda q, d: ctx.kmer_hdist_scan_dev(ref, N, k, q, d)),
                          lambda i: ctx.kmer_hdist_count_multi_dev(ref, N, k, dq, dt, nq, cm[i & 1]),
                          lambda i: ctx.kmer_hdist_count_dev(ref, N, k, int(queries[0]), int(taus[0]), one[(i & 1):(i & 1) + 1])),
                "packed": (lambda i: ctx.kmer_hdist_best_packed_async(words, nw, N, k, dq, nq, bp[i & 1], bd[i & 1]),
                           lambda i: scans(i, lambda q, d: ctx.kmer_hdist_scan_packed_dev(words, nw, N, k, q, d)),
                           lambda i: ctx.kmer_hdist_count_multi_packed_dev(words, nw, N, k, dq, dt, nq, cm[i & 1]),
                           lambda i: ctx.kmer_hdist_count_packed_dev(words, nw, N, k, int(queries[0]), int(taus[0]), one[(i & 1):(i & 1) + 1])),
            }
            for form, (best, scan_argmin, count_multi, count_one) in forms.items():
                best(0)
                scan_argmin(0)
                ctx.sync()
                equal = bool(torch.equal(bp[0], sp[0])) and bool(torch.equal(bd[0], sd[0]))
                burst, rounds = (8, 5) if nq <= 8 else ((4, 3) if nq <= 64 else (2, 2))
                a_ms = timed_sustained(torch, stream, best, burst=burst, rounds=rounds)
                b_ms = timed_sustained(torch, stream, scan_argmin, burst=burst if nq <= 8 else 1, rounds=rounds if nq <= 8 else 3)  # the median of >= 3 samples
                c_ms = timed_sustained(torch, stream, count_multi, burst=burst, rounds=rounds)
                idle = timed_queue(torch, stream, best, n_launches=8, idle_s=0.5, every=8)
                ctx.sync()
                fl = floor_ms(nq, nwin)
                run = {"k": k, "n_queries": nq, "form": form, "equal_to_scan_argmin": equal,
                       "best_burst_ms": round(a_ms, 4), "best_from_idle_ms": round(sum(idle) / len(idle), 4),
                       "scan_argmin_burst_ms": round(b_ms, 4), "best_over_scan_argmin": round(a_ms / b_ms, 4),
                       "count_multi_burst_ms": round(c_ms, 4), "best_over_count_multi": round(a_ms / c_ms, 4),
                       "matrix_floor_ms": round(fl, 4), "best_frac_of_matrix_floor": round(fl / a_ms, 4),
                       "exact_matches": int((bd[0] == 0).sum())}
                if nq == 1:
                    run["single_count_burst_ms"] = round(timed_sustained(torch, stream, count_one, burst=burst, rounds=rounds), 4)
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
            del dq, dt, bp, bd, sp, sd, cm
    doc["best_faster_than_scan_argmin_everywhere"] = all(r["equal_to_scan_argmin"] and r["best_over_scan_argmin"] < 1 for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
