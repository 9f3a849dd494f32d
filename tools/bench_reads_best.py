"""The best match per read (bitnuc_reads_hdist_best[_packed]_async, scan_reads_device.h) against the best match per query over the same bytes as ONE
sequence -- the same contraction work, the structural yardstick -- and against what the library offered before it: Q distance scans over the batch
as if it were one sequence, each followed by a masked per-read arg-min in torch, merged over the queries.  One process.

6,666,667 reads x 150 bases of the nucgen stream (seed 0xB17C0DE), encoded with encode_fixed_dev (5 words per read); k in {16, 31}; Q in
{1, 8, 64, 512} queries, half of them windows of reads (their read's best match is exact) and half random.  For each (k, Q) and input form (ASCII
bytes, packed words):
  (a) the new call;
  (b) bitnuc_kmer_hdist_best[_packed]_async over the same bytes / words as one sequence;
  (c) Q x (bitnuc_kmer_hdist_scan[_packed]_dev into a distance buffer + torch.min over the admissible columns of its (count, period) view + the
      (dist, query) merge), timed at Q <= 8 and scaled by Q beyond that (one query's cost does not depend on the others);
timed as bench.py times its config-5 block: sustained bursts of back-to-back calls (timed_sustained), (a) and (b) in alternating queues, three of
each, so that the spread of (b) stands beside the ratio (a) / (b); and, for (a), a short queue started on an idle chip (timed_queue).  The three
result arrays of (a) and (c) are compared (they must be equal).  Reported beside the times: the fraction of the matrix-pipe floor (Q x 4 MFMAs x 32
cycles per 1024 windows of the run over 1024 SIMDs at 2.4 GHz) and the admissible share of the run's windows.

    python tools/bench_reads_best.py [--out FILE] [--ks 16,31] [--qs 1,8,64,512] [--count 6666667]      one JSON document
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import timed_queue, timed_sustained  # noqa: E402

SEED = 0xB17C0DE
READ_LEN = 150
CLOCK_HZ, SIMDS = 2.4e9, 1024
SCAN_QUERIES = 8  # (c) is timed with at most this many queries


def floor_ms(q, nwin):
    return q * 4 * 32 * (nwin / 1024) / SIMDS / CLOCK_HZ * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    count, wpr = args.count, (READ_LEN + 31) // 32
    n = count * READ_LEN
    periods = {"ascii": READ_LEN, "packed": 32 * wpr}
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(count * wpr, dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, words)
    ctx.sync()
    dist = torch.empty((2, count * periods["packed"]), dtype=torch.uint8, device=dev)  # (c)'s distance bytes, alternating
    rows = torch.arange(count, device=dev)
    rng = np.random.default_rng(2028)
    doc = {"reads": count, "read_len": READ_LEN, "seed": SEED, "clock_hz_for_floor": CLOCK_HZ, "simds": SIMDS, "device": torch.cuda.get_device_name(0),
           "library": L.load().bitnuc_version().decode(), "runs": []}
    for k in [int(x) for x in args.ks.split(",")]:
        nw = READ_LEN - k + 1
        for nq in [int(x) for x in args.qs.split(",")]:
            qs = []
            for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, nw, size=(nq + 1) // 2)):
                at = int(r) * READ_LEN + int(p)
                h = ref[at:at + k].cpu().numpy()
                qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            out = [tuple(torch.zeros(count, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.uint8)) for _ in range(2)]  # (a)
            sq, sp, sd = (torch.zeros(count, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.uint8))  # (c)
            bp = torch.zeros((2, nq), dtype=torch.int64, device=dev)  # (b)
            bd = torch.zeros((2, nq), dtype=torch.uint8, device=dev)
            nsc = min(nq, SCAN_QUERIES)

            def scans(i, scan, period, m):
                """(c) for the first m queries: the masked per-read arg-min of each scan, merged in (dist, query) order"""
                sd.fill_(0xFF)
                sq.fill_(-1)
                sp.fill_(-1)
                for j in range(m):
                    d = dist[(i + j) & 1, :count * period]
                    scan(int(queries[j]), d[:count * period - k + 1])
                    v, at = torch.min(d.view(count, period)[:, :nw], dim=1)  # the first minimum of a row
                    take = v < sd
                    sd.copy_(torch.where(take, v, sd))
                    sp.copy_(torch.where(take, at.to(torch.int32), sp))
                    sq.masked_fill_(take, j)

            na, npk = n, count * periods["packed"]
            forms = {
                "ascii": (lambda i: ctx.reads_hdist_best_async(ref, READ_LEN, count, k, dq, nq, *out[i & 1]),
                          lambda i: ctx.kmer_hdist_best_async(ref, na, k, dq, nq, bp[i & 1], bd[i & 1]),
                          lambda i, m=nsc: scans(i, lambda q, d: ctx.kmer_hdist_scan_dev(ref, na, k, q, d), periods["ascii"], m)),
                "packed": (lambda i: ctx.reads_hdist_best_packed_async(words, READ_LEN, count, k, dq, nq, *out[i & 1]),
                           lambda i: ctx.kmer_hdist_best_packed_async(words, count * wpr, npk, k, dq, nq, bp[i & 1], bd[i & 1]),
                           lambda i, m=nsc: scans(i, lambda q, d: ctx.kmer_hdist_scan_packed_dev(words, count * wpr, npk, k, q, d), periods["packed"], m)),
            }
            for form, (reads_best, best_one_seq, scan_argmin) in forms.items():
                reads_best(0)
                scan_argmin(0, nq if nq <= 64 else SCAN_QUERIES)  # the equality check runs every query up to 64, the first eight beyond
                ctx.sync()
                if nq <= 64:
                    equal = all(bool(torch.equal(a, b)) for a, b in zip(out[0], (sq, sp, sd)))
                else:  # (c) saw eight queries only: (a) with those eight
                    ctx.reads_hdist_best_async(ref, READ_LEN, count, k, dq, SCAN_QUERIES, *out[1]) if form == "ascii" else \
                        ctx.reads_hdist_best_packed_async(words, READ_LEN, count, k, dq, SCAN_QUERIES, *out[1])
                    ctx.sync()
                    equal = all(bool(torch.equal(a, b)) for a, b in zip(out[1], (sq, sp, sd)))
                burst, rounds = (8, 5) if nq <= 8 else ((4, 3) if nq <= 64 else (2, 2))
                a_runs, b_runs = [], []
                for _ in range(3):  # alternating queues
                    a_runs.append(timed_sustained(torch, stream, reads_best, burst=burst, rounds=rounds))
                    b_runs.append(timed_sustained(torch, stream, best_one_seq, burst=burst, rounds=rounds))
                a_ms, b_ms = statistics.median(a_runs), statistics.median(b_runs)
                c_ms = timed_sustained(torch, stream, scan_argmin, burst=2, rounds=3) * (nq / nsc)
                idle = timed_queue(torch, stream, reads_best, n_launches=8, idle_s=0.5, every=8)
                ctx.sync()
                period = periods[form]
                fl = floor_ms(nq, count * period)
                run = {"k": k, "n_queries": nq, "form": form, "equal_to_scan_argmin": equal,
                       "reads_best_burst_ms": round(a_ms, 4), "reads_best_runs_ms": [round(x, 4) for x in a_runs],
                       "reads_best_from_idle_ms": round(sum(idle) / len(idle), 4),
                       "best_one_sequence_burst_ms": round(b_ms, 4), "best_one_sequence_runs_ms": [round(x, 4) for x in b_runs],
                       "best_one_sequence_spread": round((max(b_runs) - min(b_runs)) / b_ms, 4),
                       "reads_best_over_best_one_sequence": round(a_ms / b_ms, 4),
                       "scan_argmin_ms": round(c_ms, 4), "scan_argmin_timed_queries": nsc, "reads_best_over_scan_argmin": round(a_ms / c_ms, 4),
                       "matrix_floor_ms": round(fl, 4), "reads_best_frac_of_matrix_floor": round(fl / a_ms, 4),
                       "admissible_window_share": round(nw / period, 4), "exact_matches": int((out[0][2] == 0).sum())}
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
            del dq, out, sq, sp, sd, bp, bd
    doc["reads_best_faster_than_scan_argmin_everywhere"] = all(r["equal_to_scan_argmin"] and r["reads_best_over_scan_argmin"] < 1 for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
