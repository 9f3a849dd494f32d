"""The k-mer hit lists (bitnuc_kmer_hdist_hits_dev / _hits_packed_dev) against the fused count at the same tau, in one process.

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device; k = 31; the query is the 31-mer at base 777,777,777 (as the full-size
tests).  Timed as tools/bench_packed_scan.py: sustained bursts of 8 launches, and a queue of 32 launches started on an idle chip (groups of 8),
alternating the forms in the same process:
  * tau 3 and 8 (sparse hits): the ASCII and packed hit lists (positions and distances) next to the ASCII and packed count;
  * tau 31 (every window a hit: 8 GB of positions + 1 GB of distances), reported against HBM write bandwidth.
The hit list reads its input twice (count pass, emit pass) and writes 9 B per hit; the count reads it once and writes nothing.

    python tools/bench_kmer_hits.py [--out FILE]        one JSON document
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import timed_queue, timed_sustained  # noqa: E402

SEED = 0xB17C0DE
N, K, QPOS = 10**9, 31, 777_777_777
HBM_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import build
    build.ensure_built(build=False)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)
    nw = (N + 31) // 32
    nwin = N - K + 1
    ref = torch.empty(N, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, N, SEED)
    words = torch.zeros(nw + 2, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, N, words)
    ctx.sync()
    q = bn.as_2bit(bytes(ref[QPOS:QPOS + K].cpu().numpy()))
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    w0 = words.data_ptr()
    out = {"workload": f"{N} nucgen bases, k = {K}, query = the {K}-mer at base {QPOS}; one process, the forms alternating",
           "device": torch.cuda.get_device_name(0), "tau": {}}
    for tau in (3, 8, 31):
        ctx.kmer_hdist_count_dev(ref, N, K, q, tau, cnt)
        ctx.sync()
        total = int(cnt[0])
        cap = max(total, 1)
        pos = [torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2)]
        hd = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        forms = {
            "count_ascii": (lambda i: ctx.kmer_hdist_count_dev(ref, N, K, q, tau, cnt.data_ptr() + 8 * (i & 1))),
            "count_packed": (lambda i: ctx.kmer_hdist_count_packed_dev(w0, nw, N, K, q, tau, cnt.data_ptr() + 16 + 8 * (i & 1))),
            "hits_ascii": (lambda i: ctx.kmer_hdist_hits_dev(ref, N, K, q, tau, pos[i & 1], hd[i & 1], cap, cnt.data_ptr() + 32 + 8 * (i & 1))),
            "hits_packed": (lambda i: ctx.kmer_hdist_hits_packed_dev(w0, nw, N, K, q, tau, pos[i & 1], hd[i & 1], cap, cnt.data_ptr() + 48 + 8 * (i & 1))),
        }
        res = {"hits": total}
        for name, fn in forms.items():
            fn(0)
            ctx.sync()
            burst = timed_sustained(torch, stream, fn, burst=8, rounds=3)
            q32 = timed_queue(torch, stream, fn, n_launches=32, idle_s=1.0, every=8)
            r = {"burst_ms": round(burst, 4), "from_idle_groups_of_8_ms": [round(x, 4) for x in q32]}
            if name.startswith("hits"):
                r["written_bytes"] = 9 * total
                r["write_gbs_burst"] = round(9 * total / (burst * 1e-3) / 1e9, 1)
                r["write_frac_of_8tbs_burst"] = round(9 * total / (burst * 1e-3) / 1e9 / HBM_GBS, 4)
            res[name] = r
            ctx.sync()
        res["hits_over_count_ascii_burst"] = round(res["hits_ascii"]["burst_ms"] / res["count_ascii"]["burst_ms"], 3)
        res["hits_over_count_packed_burst"] = round(res["hits_packed"]["burst_ms"] / res["count_packed"]["burst_ms"], 3)
        out["tau"][str(tau)] = res
        del pos, hd
        torch.cuda.empty_cache()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
