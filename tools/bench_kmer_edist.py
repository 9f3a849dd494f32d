"""The indel-tolerant k-mer search along a reference (bitnuc_kmer_edist_best[_packed]_async, bitnuc_kmer_edist_count_multi[_packed]_async and the
pattern twins, scan_edist_ref_device.h) next to the Hamming forms on the same arguments and next to its own vector-issue floor.  One process.

--n bases (default 10^9) of the nucgen stream (seed 0xB17C0DE), as ASCII bytes and as packed words; k in {16, 23, 31}; Q in {1, 8, 64, 512} queries, half
of them windows of the reference and half random; best and count (tau = 2).  Per point, three alternating queues of each of
  edist     the edit-distance call
  hdist     bitnuc_kmer_hdist_best*_async / _count_multi*_dev on the same arguments (ANOTHER ANSWER: the ratio is the price of indel tolerance)
  pattern   the pattern twin on the queries' singleton patterns (the same answer as edist: one main kernel serves both kinds)
  guide     (best, Q <= 64 only) the pattern twin on guide + NGG patterns: the queries' first k - 3 bases, then N, G, G
timed as bench.py times its config-5 block (sustained bursts of back-to-back calls, timed_sustained).  Reported: the medians, each form's own spread over
its three queues ((max - min) / median), edist / hdist, pattern / edist, and the vector-issue floor: STEP_VALU vector instructions per (column, query)
-- the FAST inner loop of the shipped kernel for four interleaved queries, read from its disassembly (llvm-objdump -d of the code object, the loop of
kmer_edist_kernel<*, false> / <*, true> between its s_cbranch back edges, divided by four) -- x n x Q over CUs x 4 SIMDs x 32 lanes per clock at the
device's reported clock.  The lead-in's (1024 + 64) / 1024 is NOT in the floor: it shows in the fraction.  The outputs of edist and pattern are compared
with tests/kmer_edist_oracle.py on the first --sample bases (a call of its own on that prefix), and with each other on the whole reference.

    python tools/bench_kmer_edist.py [--out FILE] [--n 1000000000] [--ks 16,23,31] [--qs 1,8,64,512] [--sample 200000]      one JSON document
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
STEP_VALU = {"best": 20.0, "count": 20.0}  # vector instructions per (column, query) in the loop of four interleaved queries (DESIGN 3.4 has the count by opcode)
LANES_PER_CLOCK = 32  # per SIMD
TAU = 2


def spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=10**9)
    ap.add_argument("--ks", default="16,23,31")
    ap.add_argument("--qs", default="1,8,64,512")
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--sample-queries", type=int, default=4)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    import kmer_edist_oracle as ko
    import pattern_oracle as po
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    props = torch.cuda.get_device_properties(0)
    clock_hz = props.clock_rate * 1e3 if hasattr(props, "clock_rate") else 2.4e9
    simds = props.multi_processor_count * 4
    n = args.n
    nw = (n + 31) // 32
    sample = min(args.sample, n)
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, n, words)
    ctx.sync()
    head_codes = po.codes_of_ascii(ref[:sample].cpu().numpy())
    rng = np.random.default_rng(2032)
    doc = {"bases": n, "seed": SEED, "sample_bases": sample, "tau": TAU, "device": torch.cuda.get_device_name(0), "clock_mhz": clock_hz / 1e6, "simds": simds,
           "lanes_per_clock_per_simd": LANES_PER_CLOCK, "step_valu_per_query": STEP_VALU, "library": L.load().bitnuc_version().decode(), "runs": []}
    for k in [int(x) for x in args.ks.split(",")]:
        for nq in [int(x) for x in args.qs.split(",")]:
            qs = []
            for at in rng.integers(0, n - k, size=(nq + 1) // 2):
                h = ref[int(at):int(at) + k].cpu().numpy()
                qs.append(int(sum(int(((b >> 1) ^ (b >> 2)) & 3) << (2 * i) for i, b in enumerate(h))))
            qs += [int(x) for x in rng.integers(0, 2**62, size=nq // 2)]
            queries = np.array(qs, dtype=np.uint64)
            sing = ko.singletons(queries, k)
            guides = sing.copy()
            if k > 3:  # guide + NGG: the last three positions N, G, G
                for c in range(4):
                    guides[:, c] = (guides[:, c] & np.uint32((1 << (k - 3)) - 1)) | np.uint32((1 << (k - 3)) | ((3 << (k - 2)) if c == 2 else 0))
            dq = torch.from_numpy(queries.view(np.int64)).to(dev)
            dp = torch.from_numpy(sing.view(np.int32).copy()).to(dev)
            dg = torch.from_numpy(guides.view(np.int32).copy()).to(dev)
            dt = torch.full((nq,), TAU, dtype=torch.int32, device=dev)
            ends = [torch.zeros(nq, dtype=torch.int64, device=dev) for _ in range(4)]
            dists = [torch.zeros(nq, dtype=torch.uint8, device=dev) for _ in range(4)]
            sq = min(args.sample_queries, nq)
            want = ko.kmer_edist_both(head_codes, k, sing[:sq], TAU)
            for form in ("ascii", "packed"):
                src = (ref, n) if form == "ascii" else (words, nw, n)
                small = (ref, sample) if form == "ascii" else (words, (sample + 31) // 32, sample)
                sfx = "" if form == "ascii" else "_packed"
                for out in ("best", "count"):
                    if out == "best":
                        fe, fp = (getattr(ctx, f"kmer_{x}edist_best{sfx}_async") for x in ("", "pattern_"))
                        fh = getattr(ctx, f"kmer_hdist_best{sfx}_async")
                        edist = lambda i, a=src: fe(*a, k, dq, nq, ends[i & 1], dists[i & 1])
                        pattern = lambda i: fp(*src, k, dp, nq, ends[2 + (i & 1)], dists[2 + (i & 1)])
                        guide = lambda i: fp(*src, k, dg, nq, ends[2 + (i & 1)], dists[2 + (i & 1)])
                        hdist = lambda i: fh(*src, k, dq, nq, ends[2 + (i & 1)], dists[2 + (i & 1)])
                    else:
                        fe, fp = (getattr(ctx, f"kmer_{x}edist_count_multi{sfx}_async") for x in ("", "pattern_"))
                        fh = getattr(ctx, f"kmer_hdist_count_multi{sfx}_dev")
                        edist = lambda i, a=src: fe(*a, k, dq, dt, nq, ends[i & 1])
                        pattern = lambda i: fp(*src, k, dp, dt, nq, ends[2 + (i & 1)])
                        guide = None
                        hdist = lambda i: fh(*src, k, dq, dt, nq, ends[2 + (i & 1)])
                    edist(0, small)  # the prefix against the oracle
                    ctx.sync()
                    got = ends[0][:sq].cpu().numpy().view(np.uint64)
                    if out == "best":
                        equal_oracle = bool(np.array_equal(got, want[0]) and np.array_equal(dists[0][:sq].cpu().numpy(), want[1]))
                    else:
                        equal_oracle = bool(np.array_equal(got, want[2]))
                    edist(0)
                    pattern(0)
                    ctx.sync()
                    equal_pattern = bool(torch.equal(ends[0], ends[2]) and (out == "count" or torch.equal(dists[0], dists[2])))
                    whole = (ends[0].cpu().numpy().view(np.uint64).copy(), dists[0].cpu().numpy().copy())
                    hdist(0)
                    ctx.sync()
                    if out == "best":
                        against_hdist = bool((torch.from_numpy(whole[1]).to(dev) <= dists[2]).all())  # dist <= the Hamming best match's
                    else:
                        against_hdist = bool((whole[0] >= ends[2].cpu().numpy().view(np.uint64)).all())  # counts >= the Hamming count's
                    burst, rounds = (4, 2) if nq <= 8 else (2, 1) if nq <= 64 else (1, 1)
                    forms = {"edist": edist, "hdist": hdist, "pattern": pattern}
                    if guide is not None and nq <= 64 and k > 3:
                        forms["guide"] = guide
                    runs = {name: [] for name in forms}
                    for _ in range(3):  # alternating queues
                        for name, fn in forms.items():
                            runs[name].append(timed_sustained(torch, stream, fn, burst=burst, rounds=rounds))
                    ctx.sync()
                    med = {name: statistics.median(v) for name, v in runs.items()}
                    floor_ms = STEP_VALU[out] * n * nq / (simds * LANES_PER_CLOCK) / clock_hz * 1e3
                    run = {"k": k, "n_queries": nq, "form": form, "output": out, "equal_to_oracle_on_sample": equal_oracle, "pattern_equal_to_exact": equal_pattern,
                           "consistent_with_hdist": against_hdist}
                    for name in forms:
                        run[name + "_ms"] = round(med[name], 4)
                        run[name + "_runs_ms"] = [round(x, 4) for x in runs[name]]
                        run[name + "_spread"] = round(spread(runs[name]), 4)
                    run.update({"edist_over_hdist": round(med["edist"] / med["hdist"], 3), "pattern_over_edist": round(med["pattern"] / med["edist"], 4),
                                "valu_floor_ms": round(floor_ms, 4), "floor_over_edist": round(floor_ms / med["edist"], 4)})
                    doc["runs"].append(run)
                    print(json.dumps(run), flush=True)
            del dq, dp, dg, dt
    doc["all_equal"] = all(r["equal_to_oracle_on_sample"] and r["pattern_equal_to_exact"] and r["consistent_with_hdist"] for r in doc["runs"])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
