"""The sliding 31-mer Hamming scan and its fused count on PACKED words against the ASCII forms, in one process.

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device; k = 31; the query is the 31-mer at base 777,777,777 (as the full-size
tests).  Timed as bench.py's config-5 block: a queue of 96 launches started on an idle chip (groups of 8, the median of three queues) and sustained
bursts of 8 launches, alternating the forms in the same process:
  * the ASCII scan, the packed scan on 16-byte aligned words and on words at +8 bytes;
  * the ASCII count and the packed count at tau in {3, 8, 31}.
Rates: the scan at its algorithmic bytes per window (ASCII 2 B, packed 1.25 B: a quarter byte in, a byte out) against 8 TB/s; the count against
both of its floors -- HBM (ASCII 1 B, packed 0.25 B per window over 8 TB/s) and the matrix pipe (3 MFMAs x 32 cycles per 1024 windows per wave at
2.4 GHz over 1024 SIMDs) -- and which one bounds it.

    python tools/bench_packed_scan.py [--out FILE]                    one JSON document
    python tools/bench_packed_scan.py --trace-only                    96 launches of each packed kernel from an idle chip, nothing timed:
        rocprofv3 --kernel-trace --stats -f csv -d DIR -o packed -- python tools/bench_packed_scan.py --trace-only
    (build first: the library refuses to build under a profiler; without -f csv rocprofv3 writes a rocpd database whose `kernels` view
    holds the same dispatches: profiles/r06_packed_scan/kernel_stats_packed.csv and kernel_durations_packed.csv were taken from it)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import timed_queue, timed_sustained  # noqa: E402

SEED = 0xB17C0DE
N, K, QPOS = 10**9, 31, 777_777_777
HBM_GBS = 8000.0
CLOCK_HZ, SIMDS = 2.4e9, 1024


def summary(q96, burst_ms, alg_bytes):
    mean = sum(q96) / len(q96)
    settled = sum(q96[-2:]) / 2
    return {"from_idle_mean_ms": round(mean, 4), "first8_ms": round(q96[0], 4), "settled_last16_ms": round(settled, 4),
            "first_over_settled": round(q96[0] / settled, 3), "slowest_group_over_settled": round(max(q96) / settled, 3),
            "burst_ms": round(burst_ms, 4), "groups_of_8_ms": [round(x, 4) for x in q96],
            "from_idle_frac_of_8tbs": round(alg_bytes / (mean * 1e-3) / 1e9 / HBM_GBS, 4), "burst_frac_of_8tbs": round(alg_bytes / (burst_ms * 1e-3) / 1e9 / HBM_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    nw = (N + 31) // 32
    nwin = N - K + 1
    ref = torch.empty(N, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, N, SEED)
    words = torch.zeros(nw + 2, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, N, words)
    words8 = torch.zeros(nw + 2, dtype=torch.int64, device=dev)
    words8[1:nw + 1] = words[:nw]
    ctx.sync()
    q = bn.as_2bit(bytes(ref[QPOS:QPOS + K].cpu().numpy()))
    dists = [torch.empty(nwin, dtype=torch.uint8, device=dev) for _ in range(2)]
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    w0, w8 = words.data_ptr(), words8.data_ptr() + 8

    scan = {
        "ascii": (lambda i: ctx.kmer_hdist_scan_dev(ref, N, K, q, dists[i & 1]), 2 * nwin),
        "packed": (lambda i: ctx.kmer_hdist_scan_packed_dev(w0, nw, N, K, q, dists[i & 1]), 1.25 * nwin),
        "packed_words_plus8": (lambda i: ctx.kmer_hdist_scan_packed_dev(w8, nw, N, K, q, dists[i & 1]), 1.25 * nwin),
    }

    def count_forms(tau):
        return {"ascii": (lambda i: ctx.kmer_hdist_count_dev(ref, N, K, q, tau, cnt), nwin),
                "packed": (lambda i: ctx.kmer_hdist_count_packed_dev(w0, nw, N, K, q, tau, cnt.data_ptr() + 8), 0.25 * nwin),
                "packed_words_plus8": (lambda i: ctx.kmer_hdist_count_packed_dev(w8, nw, N, K, q, tau, cnt.data_ptr() + 16), 0.25 * nwin)}

    if args.trace_only:
        for fn, _ in (scan["packed"], count_forms(8)["packed"]):
            torch.cuda.synchronize()
            time.sleep(1.0)
            for i in range(96):
                fn(i)
        torch.cuda.synchronize()
        ctx.close()
        return

    # correctness before timing: the packed forms agree with the ASCII ones on this input
    scan["ascii"][0](0)
    for name in ("packed", "packed_words_plus8"):
        dists[1].zero_()
        scan[name][0](1)
        ctx.sync()
        assert torch.equal(dists[0], dists[1]), name
    for tau in (3, 8, 31):
        for name, (fn, _) in count_forms(tau).items():
            fn(0)
        ctx.sync()
        assert int(cnt[1]) == int(cnt[2]) == int(cnt[0]), (tau, cnt.tolist())

    def measure(forms):
        out = {name: [] for name in forms}
        bursts = {name: [] for name in forms}
        for _ in range(3):  # alternate the forms: each queue starts after its own second of idleness
            for name, (fn, _) in forms.items():
                out[name].append(timed_queue(torch, stream, fn, n_launches=96, idle_s=1.0, every=8))
                bursts[name].append(timed_sustained(torch, stream, fn))
        res = {}
        for name, (_, alg) in forms.items():
            q96 = sorted(out[name], key=sum)[1]  # the queue with the median mean
            res[name] = summary(q96, sorted(bursts[name])[1], alg)
            res[name]["from_idle_means_of_three_ms"] = [round(sum(x) / len(x), 4) for x in out[name]]
        return res

    result = {"tool": "tools/bench_packed_scan.py", "n_bases": N, "k": K, "query_at": QPOS, "seed": SEED, "csrc_sha16": build.csrc_sha16(),
              "device": torch.cuda.get_device_name(0)}
    result["scan"] = measure(scan)
    s = result["scan"]
    s["packed_over_ascii_from_idle"] = round(s["packed"]["from_idle_mean_ms"] / s["ascii"]["from_idle_mean_ms"], 3)
    s["plus8_over_aligned_from_idle"] = round(s["packed_words_plus8"]["from_idle_mean_ms"] / s["packed"]["from_idle_mean_ms"], 3)
    s["scan_hbm_floor_ms_packed"] = round(1.25 * nwin / (HBM_GBS * 1e9) * 1e3, 4)
    hbm_floor = 0.25 * nwin / (HBM_GBS * 1e9) * 1e3
    mfma_floor = (nwin / 1024) * 3 * 32 / (SIMDS * CLOCK_HZ) * 1e3
    result["count_floors_ms"] = {"hbm_0.25B_per_window": round(hbm_floor, 4), "matrix_pipe_3x32_cycles": round(mfma_floor, 4),
                                 "bound": "matrix pipe" if mfma_floor > hbm_floor else "hbm"}
    result["count"] = {}
    for tau in (3, 8, 31):
        r = measure(count_forms(tau))
        r["packed_over_ascii_from_idle"] = round(r["packed"]["from_idle_mean_ms"] / r["ascii"]["from_idle_mean_ms"], 3)
        r["plus8_over_aligned_from_idle"] = round(r["packed_words_plus8"]["from_idle_mean_ms"] / r["packed"]["from_idle_mean_ms"], 3)
        for name in ("packed", "packed_words_plus8"):
            r[name]["frac_of_matrix_floor"] = round(mfma_floor / r[name]["from_idle_mean_ms"], 4)
            r[name]["frac_of_hbm_floor"] = round(hbm_floor / r[name]["from_idle_mean_ms"], 4)
        result["count"][f"tau_{tau}"] = r
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"scan_packed_over_ascii": s["packed_over_ascii_from_idle"], "scan_plus8_over_aligned": s["plus8_over_aligned_from_idle"],
                      "count_packed_over_ascii": {t: v["packed_over_ascii_from_idle"] for t, v in result["count"].items()}}))
    ctx.close()


if __name__ == "__main__":
    main()
