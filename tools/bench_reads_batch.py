"""The best match per read of a RAGGED batch (bitnuc_reads_hdist_best_batch[_packed]_async, scan_reads_batch_device.h) against the fixed-length forms on
the same bytes, on ragged lengths with and without reads shorter than a segment, and against what the library offered before it: Q distance scans
over the concatenation, each followed by a masked per-read arg-min in torch, merged over the queries.  One process.

About 10^9 bases of the nucgen stream (seed 0xB17C0DE), packed with encode_batch_dev; k = 31; Q in {1, 8, 64, 512} queries, half of them windows of
the batch and half random; ASCII bytes and packed words.  Three batches:
  fixed     6,666,667 reads x 150 bases: the ragged entry points against bitnuc_reads_hdist_best[_packed]_async on the same bytes (results must be
            equal; the ratio is the cost of the table lookup);
  ragged    lengths uniform in [100, 200]: the fast path on ragged lengths;
  short5    the same with 5 % of the reads replaced by reads of 1 .. 31 bases: the exact path, ASCII against packed;
and for each, today's route (d): Q x (bitnuc_kmer_hdist_scan[_packed]_dev over the concatenation into a distance buffer + one scatter-min of
(distance, offset) keys over the windows that end inside their read + the (dist, query) merge), timed at Q = 1 and at 8 queries and scaled by Q
beyond that (the timing at 8 queries is taken once per batch and form, in the first run with 8 or more queries, and reused), its three result arrays compared with the ragged
form's at every Q (they must be equal).
Timed as bench.py times its config-5 block: sustained bursts of back-to-back calls (timed_sustained; (d), hundreds of launches long, one call at a
time); the ragged form, the fixed-length form (on the
batch of equal lengths) and (d) in alternating queues, three of each, every form's own spread beside its median.

    python tools/bench_reads_batch.py [--out FILE] [--qs 1,8,64,512] [--bases 1000000000] [--batches fixed,ragged,short5]      one JSON document
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import timed_sustained  # noqa: E402

SEED = 0xB17C0DE
K = 31
SCAN_QUERIES = 8  # (d) is timed with at most this many queries


def lengths_of(batch, bases, rng):
    if batch == "fixed":
        return np.full(bases // 150, 150, dtype=np.int64)
    lens = rng.integers(100, 201, size=bases // 150)
    if batch == "short5":
        short = rng.random(lens.size) < 0.05
        lens[short] = rng.integers(1, 32, size=int(short.sum()))
    return lens.astype(np.int64)


def spread(runs):
    return round((max(runs) - min(runs)) / statistics.median(runs), 4)


def timed_once(torch, stream, fn):
    """ms of one call of a long-running composite (seconds of back-to-back launches: no burst needed to hide a launch gap)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--bases", type=int, default=1_000_000_050)
    ap.add_argument("--batches", default="fixed,ragged,short5")
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    rng = np.random.default_rng(2029)
    d_cache = {}
    doc = {"k": K, "seed": SEED, "device": torch.cuda.get_device_name(0), "library": L.load().bitnuc_version().decode(), "runs": []}
    for batch in args.batches.split(","):
        lens = lengths_of(batch, args.bases, rng)
        count = lens.size
        off = np.zeros(count + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        wo = np.zeros(count + 1, dtype=np.int64)
        wo[1:] = np.cumsum((lens + 31) // 32)
        n, nw = int(off[-1]), int(wo[-1])
        d_off, d_wo = torch.from_numpy(off).to(dev), torch.from_numpy(wo).to(dev)
        ref = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.nucgen_dev(ref, n, SEED)
        words = torch.zeros(nw, dtype=torch.int64, device=dev)
        ctx.encode_batch_dev(ref, d_off, d_wo, count, nw, words)
        ctx.sync()
        # (d)'s precomputed side: per window of each run its read, its offset in the read, and whether it ends inside the read
        runs = {}
        for form, starts, total in (("ascii", d_off, n), ("packed", d_wo * 32, 32 * nw)):
            live = torch.nonzero(starts[1:] > starts[:-1]).reshape(-1)
            read_of = torch.repeat_interleave(live, (starts[live + 1] - starts[live]))  # the run's windows in order: only reads that own windows
            local = torch.arange(total, device=dev) - starts[read_of]
            masked = local + K > (d_off[read_of + 1] - d_off[read_of])
            runs[form] = (read_of, local, masked, total)
            del live
        dist = torch.empty(32 * nw, dtype=torch.uint8, device=dev)
        for nq in [int(x) for x in args.qs.split(",")]:
            at = rng.integers(0, n - K, size=(nq + 1) // 2)
            qs = []
            for a in at:
                h = ref[int(a):int(a) + K].cpu().numpy()
                qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            out = [tuple(torch.zeros(count, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.uint8)) for _ in range(2)]
            fix = tuple(torch.zeros(count, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.uint8))
            best = torch.empty(count, dtype=torch.int64, device=dev)
            sq, sp, sd = (torch.zeros(count, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.uint8))
            nsc = min(nq, SCAN_QUERIES)

            def scans(form, m):
                """(d) for the first m queries: the per-read minimum of (distance, offset) over each scan's admissible windows, merged in query order"""
                read_of, local, masked, total = runs[form]
                sd.fill_(0xFF)
                sq.fill_(-1)
                sp.fill_(-1)
                for j in range(m):
                    d = dist[:total]
                    if form == "ascii":
                        ctx.kmer_hdist_scan_dev(ref, n, K, int(queries[j]), d[:n - K + 1])
                    else:
                        ctx.kmer_hdist_scan_packed_dev(words, nw, 32 * nw, K, int(queries[j]), d[:32 * nw - K + 1])
                    key = torch.where(masked, 0xFF, d.to(torch.int64)) << 32 | local
                    best.fill_(0xFF << 32)
                    best.scatter_reduce_(0, read_of, key, "amin")
                    v = (best >> 32).to(torch.uint8)
                    take = v < sd
                    sd.copy_(torch.where(take, v, sd))
                    sp.copy_(torch.where(take, (best & 0xFFFFFFFF).to(torch.int32), sp))
                    sq.masked_fill_(take, j)
                    del key

            calls = {
                "ascii": (lambda i, q=nq: ctx.reads_hdist_best_batch_async(ref, d_off, count, n, K, dq, q, *out[i & 1]),
                          lambda i: ctx.reads_hdist_best_async(ref, 150, count, K, dq, nq, *fix)),
                "packed": (lambda i, q=nq: ctx.reads_hdist_best_batch_packed_async(words, d_wo, d_off, count, nw, K, dq, q, *out[i & 1]),
                           lambda i: ctx.reads_hdist_best_packed_async(words, 150, count, K, dq, nq, *fix)),
            }
            for form, (ragged, fixed) in calls.items():
                ragged(0)
                ctx.sync()
                run = {"batch": batch, "reads": count, "bases": n, "n_queries": nq, "form": form}
                if batch == "fixed":
                    fixed(0)
                    ctx.sync()
                    run["equal_to_fixed_length_form"] = all(bool(torch.equal(a, b)) for a, b in zip(out[0], fix))
                ragged(1, nsc)  # (d) sees nsc queries: the ragged form with those
                scans(form, nsc)
                ctx.sync()
                run["equal_to_scan_argmin"] = all(bool(torch.equal(a, b)) for a, b in zip(out[1], (sq, sp, sd)))
                burst, rounds = (8, 4) if nq <= 8 else ((4, 3) if nq <= 64 else (2, 2))
                timed_d = (batch, form, nsc) not in d_cache  # one query's cost does not depend on Q: (d) at 8 queries is timed once per batch and form
                a_runs, f_runs, d_runs = [], [], []
                for _ in range(3):  # alternating queues: the ragged form, the fixed-length form (the batch of equal lengths), (d)
                    a_runs.append(timed_sustained(torch, stream, ragged, burst=burst, rounds=rounds))
                    if batch == "fixed":
                        f_runs.append(timed_sustained(torch, stream, fixed, burst=burst, rounds=rounds))
                    if timed_d:
                        d_runs.append(timed_once(torch, stream, lambda: scans(form, nsc)) / nsc)  # (warm: the equality check ran it)
                if timed_d:
                    d_cache[(batch, form, nsc)] = d_runs
                d_runs = [x * nq for x in d_cache[(batch, form, nsc)]]  # per query, scaled by Q
                a_ms, d_ms = statistics.median(a_runs), statistics.median(d_runs)
                run["scan_argmin_timed_in_this_run"] = timed_d
                run.update({"ragged_ms": round(a_ms, 4), "ragged_runs_ms": [round(x, 4) for x in a_runs], "ragged_spread": spread(a_runs),
                            "scan_argmin_ms": round(d_ms, 4), "scan_argmin_runs_ms": [round(x, 4) for x in d_runs], "scan_argmin_spread": spread(d_runs),
                            "scan_argmin_timed_queries": nsc, "ragged_over_scan_argmin": round(a_ms / d_ms, 4),
                            "faster_than_scan_argmin_by_more_than_both_spreads": max(a_runs) < min(d_runs),
                            "exact_matches": int((out[0][2] == 0).sum())})
                if batch == "fixed":
                    f_ms = statistics.median(f_runs)
                    run.update({"fixed_ms": round(f_ms, 4), "fixed_runs_ms": [round(x, 4) for x in f_runs], "fixed_spread": spread(f_runs),
                                "ragged_over_fixed": round(a_ms / f_ms, 4)})
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
            del dq, out, fix, best, sq, sp, sd
        del ref, words, dist, runs, d_off, d_wo
        torch.cuda.empty_cache()
    doc["ragged_faster_than_scan_argmin_everywhere"] = all(r["equal_to_scan_argmin"] and r["faster_than_scan_argmin_by_more_than_both_spreads"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
