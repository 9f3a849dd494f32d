"""The indel-tolerant anchored match per read (bitnuc_reads_edist_anchored[_packed]_async and the pattern twins, scan_edist_device.h) next to the Hamming
form on the same arguments and next to its own vector-issue floor.  One process.

6,666,667 reads x 150 bases of the nucgen stream (seed 0xB17C0DE), encoded with encode_fixed_dev (5 words per read); k in {16, 31}; a 3' anchor with
four and eight offsets (pos_lo = 150 - k - 3 / - 7, pos_hi = to the end: spans of k + 3 and k + 7 bases); Q in {1, 8, 64, 512} queries, half of them
windows of reads inside the span and half random; ASCII bytes and packed words; six outputs.  Per point, three alternating queues of each of
  edist     the edit-distance call
  hdist     bitnuc_reads_hdist_anchored*_async on the same arguments (ANOTHER ANSWER: the ratio is the price of indel tolerance, not a speed-up)
  pattern   the pattern twin on the queries' singleton patterns (the same answer as edist)
timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported: the medians, each form's own spread over
its three queues ((max - min) / median), edist / hdist, pattern / edist, and the vector-issue floor: STEP_VALU vector instructions per (read, query,
span base) -- the inner loop of the shipped kernel, read from its disassembly: 80 for four interleaved queries -- x reads x n x Q over 256 CUs x 4 SIMDs
x 32 lanes per clock at the device's reported clock.  The six arrays of edist and pattern are compared with tests/reads_edist_oracle.py on the first
--sample reads, and with each other on all reads.

    python tools/bench_reads_edist.py [--out FILE] [--ks 16,31] [--offsets 4,8] [--qs 1,8,64,512] [--count 6666667] [--sample 64]      one JSON document
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
STEP_VALU = 20.0  # vector instructions per (read, query, span base): 80 in the loop of four interleaved queries (scan_edist_device.h)
LANES_PER_CLOCK = 32  # per SIMD


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default="16,31")
    ap.add_argument("--offsets", default="4,8")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--count", type=int, default=6_666_667)
    ap.add_argument("--sample", type=int, default=64)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import reads_edist_oracle as eo
    import reads_pattern_oracle as rp
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    props = torch.cuda.get_device_properties(0)
    clock_hz = props.clock_rate * 1e3 if hasattr(props, "clock_rate") else 2.4e9
    simds = props.multi_processor_count * 4
    count, wpr = args.count, (READ_LEN + 31) // 32
    n_bases = count * READ_LEN
    sample = min(args.sample, count)
    ref = torch.empty(n_bases, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n_bases, SEED)
    words = torch.zeros(count * wpr, dtype=torch.int64, device=dev)
    ctx.encode_fixed_dev(ref, READ_LEN, READ_LEN, count, words)
    ctx.sync()
    head = ref[:sample * READ_LEN].cpu().numpy()
    rng = np.random.default_rng(2031)
    doc = {"reads": count, "read_len": READ_LEN, "seed": SEED, "sample_reads": sample, "device": torch.cuda.get_device_name(0), "clock_mhz": clock_hz / 1e6,
           "simds": simds, "lanes_per_clock_per_simd": LANES_PER_CLOCK, "step_valu_per_query": STEP_VALU, "library": L.load().bitnuc_version().decode(), "runs": []}
    types = (torch.int32, torch.int32, torch.uint8)
    six = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    alt = [tuple(torch.zeros(count, dtype=t, device=dev) for t in types + types) for _ in range(2)]
    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            for noff in [int(x) for x in args.offsets.split(",")]:
                n = noff + k - 1
                pos_lo, pos_hi = READ_LEN - n, None
                qs = []
                for r, p in zip(rng.integers(0, count, size=(nq + 1) // 2), rng.integers(0, noff, size=(nq + 1) // 2)):
                    at = int(r) * READ_LEN + pos_lo + int(p)
                    h = ref[at:at + k].cpu().numpy()
                    qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
                qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
                queries = np.array(qs, dtype=np.uint64)
                dq = torch.from_numpy(queries.view(np.int64)).to(dev)
                dp = torch.from_numpy(rp.singletons(queries, k).view(np.int32).copy()).to(dev)
                want = eo.reads_edist(head, READ_LEN, sample, k, queries, pos_lo, pos_hi)
                floor_ms = STEP_VALU * count * n * nq / (simds * LANES_PER_CLOCK) / clock_hz * 1e3
                for form in ("ascii", "packed"):
                    src = ref if form == "ascii" else words
                    sfx = "" if form == "ascii" else "_packed"
                    fe, fh, fp = (getattr(ctx, f"reads_{x}_anchored{sfx}_async") for x in ("edist", "hdist", "pattern_edist"))
                    edist = lambda i: fe(src, READ_LEN, count, k, dq, nq, *six[i & 1], pos_lo=pos_lo, pos_hi=pos_hi)
                    hdist = lambda i: fh(src, READ_LEN, count, k, dq, nq, *alt[i & 1], pos_lo=pos_lo, pos_hi=pos_hi)
                    pattern = lambda i: fp(src, READ_LEN, count, k, dp, nq, *alt[i & 1], pos_lo=pos_lo, pos_hi=pos_hi)
                    for a in six[0] + alt[0]:
                        a.fill_(0x5A)
                    edist(0)
                    pattern(0)
                    ctx.sync()
                    got = [a[:sample].cpu().numpy() for a in six[0]]
                    equal_oracle = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
                    equal_pattern = all(bool(torch.equal(a, b)) for a, b in zip(six[0], alt[0]))
                    hdist(0)
                    ctx.sync()
                    never_above = bool((six[0][2] <= alt[0][2]).all())  # best_dist <= the Hamming form's on every read
                    below = float((six[0][2] < alt[0][2]).float().mean())
                    burst, rounds = (8, 3) if nq <= 64 else (2, 1)
                    runs = {"edist": [], "hdist": [], "pattern": []}
                    for _ in range(3):  # alternating queues
                        runs["edist"].append(timed_sustained(torch, stream, edist, burst=burst, rounds=rounds))
                        runs["hdist"].append(timed_sustained(torch, stream, hdist, burst=burst, rounds=rounds))
                        runs["pattern"].append(timed_sustained(torch, stream, pattern, burst=burst, rounds=rounds))
                    ctx.sync()
                    med = {name: statistics.median(v) for name, v in runs.items()}
                    run = {"k": k, "n_queries": nq, "offsets": noff, "pos_lo": pos_lo, "span": n, "form": form, "equal_to_oracle_on_sample": equal_oracle,
                           "pattern_equal_to_exact": equal_pattern, "never_above_hdist": never_above, "reads_below_hdist": round(below, 4)}
                    for name in ("edist", "hdist", "pattern"):
                        run[name + "_ms"] = round(med[name], 4)
                        run[name + "_runs_ms"] = [round(x, 4) for x in runs[name]]
                        run[name + "_spread"] = round(spread(runs[name]), 4)
                    run.update({"edist_over_hdist": round(med["edist"] / med["hdist"], 3), "pattern_over_edist": round(med["pattern"] / med["edist"], 4),
                                "valu_floor_ms": round(floor_ms, 4), "floor_over_edist": round(floor_ms / med["edist"], 4)})
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
                del dq, dp
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["pattern_equal_to_exact"] and r["never_above_hdist"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
