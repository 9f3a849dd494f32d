"""The anchored best match and runner-up per read (bitnuc_reads_hdist_anchored[_packed]_async, scan_anchored_device.h) against today's equal-result route
and against two computed floors.  One process.

6,666,667 reads x 150 bases of the nucgen stream (seed 0xB17C0DE), encoded with encode_fixed_dev (5 words per read); k in {16, 31}; 1 or 4 offsets at
the start (pos_lo = 0) or at the 3' end (pos_hi = to the end); Q in {1, 8, 64, 512} queries, half of them windows of reads at an admissible offset and
half random; ASCII bytes and packed words; with and without the second triple.  Per point, three alternating queues of each of
  new          the anchored call
  route        today's equal-result route on the same kernels as before: a device copy of the spans into a compact batch (ASCII: a strided torch copy;
               packed: encode_fixed_dev of the spans, read_len = span and stride = 150 -- a caller that holds only packed words has no device route)
               followed by reads_hdist_best2[_packed]_async (reads_hdist_best*_async without the second triple) on it
  route_scan   that call alone on a compact batch made beforehand (the copy's share = route - route_scan)
timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported: the medians, each form's own spread over
its three queues ((max - min) / median), new / route, and whether new is faster than route by more than the two spreads added together.  Context, once
per (k, Q, form): reads_hdist_best2*_async over the WHOLE reads (other results: a caller without the workaround runs this).
Floors, next to each time: the matrix pipe's (the kernel's MFMA count x 32 cycles over the chip's SIMDs at the device's reported clock) and memory's (the
128-byte lines the spans touch, at 8 TB/s).  The six (three) arrays are compared with tests/reads_anchored_oracle.py on the first --sample reads and
with the route's on all reads.

    python tools/bench_reads_anchored.py [--out FILE] [--ks 16,31] [--offsets 1,4] [--qs 1,8,64,512] [--count 6666667] [--sample 256]      one JSON document
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
HBM = 8.0e12  # bytes / s


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def lines_touched(count, stride_bytes, first, nbytes):
    """128-byte lines that hold a byte of [r * stride + first, + nbytes) for some read r"""
    a = (np.arange(count, dtype=np.int64) * stride_bytes + first) >> 7
    b = (np.arange(count, dtype=np.int64) * stride_bytes + first + nbytes - 1) >> 7
    return int(np.unique(np.concatenate([a, b])).size) if nbytes <= 129 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--offsets", default="1,4")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=256)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_anchored_oracle as ra
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    props = torch.cuda.get_device_properties(0)
    clock_hz = props.clock_rate * 1e3 if hasattr(props, "clock_rate") else 2.4e9
    simds = props.multi_processor_count * 4
    count, wpr = args.count, (READ_LEN + 31) // 32
    n = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(count * wpr, dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, words)
    ctx.sync()
    head = ref[:sample * READ_LEN].cpu().numpy()
    rng = np.random.default_rng(2030)
    doc = {"reads": count, "read_len": READ_LEN, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0),
           "clock_mhz": clock_hz / 1e6, "simds": simds, "hbm_bytes_per_s": HBM, "library": L.load().bitnuc_version().decode(), "runs": [], "whole_reads": []}
    types = (torch.int32, torch.int32, torch.uint8)
    six = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    alt = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    ref2d = ref.view(count, READ_LEN)
    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            for noff in [int(x) for x in args.offsets.split(",")]:
                span = noff + k - 1
                swpr = (span + 31) // 32
                for anchor in ("start", "3prime"):
                    pos_lo = 0 if anchor == "start" else READ_LEN - k - (noff - 1)
                    pos_hi = noff - 1 if anchor == "start" else None
                    qs = []
                    for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, noff, size=(nq + 1) // 2)):
                        at = int(r) * READ_LEN + pos_lo + int(p)
                        h = ref[at:at + k].cpu().numpy()
                        qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
                    qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
                    queries = np.array(qs, dtype=np.uint64)
                    dq = torch.from_numpy(queries.view(np.int64)).to(dev)
                    want = ra.reads_anchored(head, READ_LEN, sample, k, queries, pos_lo, pos_hi)
                    compact = [torch.empty((count, span), dtype=torch.uint8, device=dev) for _ in range(2)]
                    cwords = [torch.zeros(count * swpr, dtype=torch.int64, device=dev) for _ in range(2)]
                    lg = max(noff - 1, 0).bit_length()
                    mfma = ((count + 63) // 64) * 2 * (((nq << lg) + 31) // 32) * ((span + 15) // 16)
                    pipe_ms = mfma * 32 / simds / clock_hz * 1e3
                    for form in ("ascii", "packed"):
                        src = ref if form == "ascii" else words
                        if form == "ascii":
                            nlines = lines_touched(count, READ_LEN, pos_lo, span)
                        else:
                            b0, b1 = pos_lo // 4, (pos_lo + span - 1) // 4
                            nlines = lines_touched(count, wpr * 8, b0, b1 - b0 + 1)
                        mem_ms = nlines * 128 / HBM * 1e3
                        for second in (True, False):
                            nout = 6 if second else 3
                            if form == "ascii":
                                new = lambda i: ctx.reads_hdist_anchored_async(src, READ_LEN, count, k, dq, nq, *six[i & 1][:nout], pos_lo=pos_lo, pos_hi=pos_hi)
                                scan_fn = ctx.reads_hdist_best2_async if second else ctx.reads_hdist_best_async
                                copy = lambda i: compact[i & 1].copy_(ref2d[:, pos_lo:pos_lo + span])
                                scan = lambda i: scan_fn(compact[i & 1], span, count, k, dq, nq, *alt[i & 1][:nout])
                            else:
                                new = lambda i: ctx.reads_hdist_anchored_packed_async(src, READ_LEN, count, k, dq, nq, *six[i & 1][:nout], pos_lo=pos_lo, pos_hi=pos_hi)
                                scan_fn = ctx.reads_hdist_best2_packed_async if second else ctx.reads_hdist_best_packed_async
                                copy = lambda i: ctx.encode_fixed_dev(ref.data_ptr() + pos_lo, span, READ_LEN, count, cwords[i & 1])
                                scan = lambda i: scan_fn(cwords[i & 1], span, count, k, dq, nq, *alt[i & 1][:nout])

                            def route(i):
                                copy(i)
                                scan(i)
                            for a in six[0] + alt[0]:
                                a.fill_(0x5A)
                            new(0)
                            route(0)
                            copy(1)
                            ctx.sync()
                            got = [a[:sample].cpu().numpy() for a in six[0][:nout]]
                            equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
                            equal_route = True
                            for j, (a, b) in enumerate(zip(six[0][:nout], alt[0][:nout])):
                                if j % 3 == 1:  # positions: the route's are relative to pos_lo
                                    b = torch.where(b == -1, b, b + pos_lo)
                                equal_route = equal_route and bool(torch.equal(a, b))
                            burst, rounds = (8, 3) if nq <= 64 else (4, 2)
                            runs = {"new": [], "route": [], "route_scan": []}
                            for _ in range(3):  # alternating queues
                                runs["new"].append(timed_sustained(torch, stream, new, burst=burst, rounds=rounds))
                                runs["route"].append(timed_sustained(torch, stream, route, burst=burst, rounds=rounds))
                                runs["route_scan"].append(timed_sustained(torch, stream, scan, burst=burst, rounds=rounds))
                            ctx.sync()
                            med = {name: statistics.median(v) for name, v in runs.items()}
                            floor_ms = max(pipe_ms, mem_ms)
                            run = {"k": k, "n_queries": nq, "offsets": noff, "anchor": anchor, "pos_lo": pos_lo, "span": span, "form": form, "second": second,
                                   "equal_to_oracle_on_sample": equal_oracle, "equal_to_route": equal_route,
                                   "new_ms": round(med["new"], 4), "new_runs_ms": [round(x, 4) for x in runs["new"]], "new_spread": round(spread(runs["new"]), 4),
                                   "route_ms": round(med["route"], 4), "route_runs_ms": [round(x, 4) for x in runs["route"]],
                                   "route_spread": round(spread(runs["route"]), 4),
                                   "route_scan_ms": round(med["route_scan"], 4), "route_copy_ms": round(med["route"] - med["route_scan"], 4),
                                   "new_over_route": round(med["new"] / med["route"], 4),
                                   "faster_beyond_spreads": bool(med["route"] - med["new"] > (spread(runs["new"]) * med["new"] + spread(runs["route"]) * med["route"])),
                                   "mfma": mfma, "pipe_floor_ms": round(pipe_ms, 4), "lines_128B": nlines, "memory_floor_ms": round(mem_ms, 4),
                                   "binding_floor": "pipe" if pipe_ms >= mem_ms else "memory", "floor_over_new": round(floor_ms / med["new"], 4)}
                            doc["runs"].append(run)
                            print(json.dumps(run), flush=True)
                    del compact, cwords, dq
        for nq in [int(x) for x in args.qs.split(",")]:  # context: the whole reads (other results)
            queries = np.array([int(x) for x in rng.integers(0, 2**62, size=nq)], dtype=np.uint64)
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            for form in ("ascii", "packed"):
                fn = ctx.reads_hdist_best2_async if form == "ascii" else ctx.reads_hdist_best2_packed_async
                src = ref if form == "ascii" else words
                whole = lambda i: fn(src, READ_LEN, count, k, dq, nq, *alt[i & 1])
                burst, rounds = (4, 2) if nq <= 64 else (2, 1)
                ms = timed_sustained(torch, stream, whole, burst=burst, rounds=rounds)
                row = {"k": k, "n_queries": nq, "form": form, "best2_whole_reads_ms": round(ms, 4)}
                doc["whole_reads"].append(row)
                print(json.dumps(row), flush=True)
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["equal_to_route"] for r in doc["runs"])
    doc["all_faster_beyond_spreads"] = all(r["faster_beyond_spreads"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
