"""The multi-query k-mer count (bitnuc_kmer_hdist_count_multi[_packed]_dev, scan_multi_device.h) against Q single-query count calls, in one process
(DESIGN 3.4).

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device; k in {20, 31}; Q in {1, 8, 64, 512} queries, half of them windows of the
sequence (so they hit) and half random, at thresholds cycling through 0, 3, 8, k.  For each (k, Q) and input form (ASCII bytes, packed words):
  * the multi-query call, and the same Q queries as Q calls of the single-query device count (bitnuc_kmer_hdist_count[_packed]_dev), timed as bench.py
    times its config-5 block: sustained bursts of back-to-back calls (timed_sustained) and a short queue started on an idle chip (timed_queue);
  * the counts of both ways compared (they must be equal);
  * the fraction of the matrix-pipe floor: Q x 3 MFMAs x 32 cycles per 1024 windows over 1024 SIMDs at 2.4 GHz (Q x 38.1 us per 10^9 windows).

    python tools/bench_kmer_multi.py [--out FILE] [--ks 20,31] [--qs 1,8,64,512]      one JSON document
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
    return q * 3 * 32 * (nwin / 1024) / SIMDS / CLOCK_HZ * 1e3


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
    rng = np.random.default_rng(2026)
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
            cm = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            cs = torch.zeros((2, nq), dtype=torch.int64, device=dev)
            forms = {
                "ascii": (lambda i: ctx.kmer_hdist_count_multi_dev(ref, N, k, dq, dt, nq, cm[i & 1]),
                          lambda i: [ctx.kmer_hdist_count_dev(ref, N, k, int(queries[j]), int(taus[j]), cs[i & 1, j:j + 1]) for j in range(nq)]),
                "packed": (lambda i: ctx.kmer_hdist_count_multi_packed_dev(words, nw, N, k, dq, dt, nq, cm[i & 1]),
                           lambda i: [ctx.kmer_hdist_count_packed_dev(words, nw, N, k, int(queries[j]), int(taus[j]), cs[i & 1, j:j + 1]) for j in range(nq)]),
            }
            for form, (multi, single) in forms.items():
                multi(0)
                single(0)
                ctx.sync()
                equal = bool(torch.equal(cm[0], cs[0]))
                burst, rounds = (8, 5) if nq <= 8 else ((4, 3) if nq <= 64 else (2, 2))
                m_ms = timed_sustained(torch, stream, multi, burst=burst, rounds=rounds)
                s_ms = timed_sustained(torch, stream, single, burst=max(1, burst // 4) if nq >= 64 else burst, rounds=rounds)
                idle = timed_queue(torch, stream, multi, n_launches=8, idle_s=0.5, every=8)
                ctx.sync()
                fl = floor_ms(nq, nwin)
                run = {"k": k, "n_queries": nq, "form": form, "counts_equal_single": equal,
                       "multi_burst_ms": round(m_ms, 4), "multi_from_idle_ms": round(sum(idle) / len(idle), 4),
                       "singles_burst_ms": round(s_ms, 4), "multi_over_singles": round(m_ms / s_ms, 4),
                       "matrix_floor_ms": round(fl, 4), "multi_frac_of_matrix_floor": round(fl / m_ms, 4),
                       "hits_of_first_query": int(cm[0, 0])}
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
            del dq, dt, cm, cs
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
