"""The pattern queries (bitnuc_kmer_pattern_count_multi / _best / _hits [_packed] _async) against their exact twins in one process, and the exact
forms of this tree against the same forms of another tree (the parent commit) measured in the same visit.

10^9 bases of the nucgen stream (seed 0xB17C0DE), encoded on the device; k = 23; Q in {1, 64, 512} queries.  A pattern is twenty exact bases + NGG
(the guide search), half of the guides windows of the sequence and half random; its exact twin is the same guide + AGG.  Thresholds cycle through
0, 3, 8, k.  The hit lists take one query at tau = 3.  For each family (count_multi, best, hits), input form (ASCII bytes, packed words) and Q:
five queues of back-to-back calls of the pattern form ALTERNATING with five of the exact form (device events around each queue, one call of warm-up
before it), so that the exact form's own queue-to-queue spread is on record beside the ratio.  Before anything is timed, the pattern forms are run on the
SINGLETON patterns of the exact queries and must return exactly what the exact forms return (asserted).

    python tools/bench_kmer_pattern.py --out FILE                                   this tree, pattern and exact forms
    python tools/bench_kmer_pattern.py --exact-only --tree DIR --out FILE           another tree's exact forms (DIR holds its bitnuc_amd/ and include/)
    python tools/bench_kmer_pattern.py --fold FILE --parent FILE [--parent FILE] --out FILE     no measurement: fold the other tree's documents
                                                                                    (taken before and after this tree's) into this tree's

One JSON document.  ratio = median(pattern) / median(exact); spread = (max - min) / median over a form's five queues.  `exact_vs_parent`: this tree's
exact median over the parent's, beside the parent's spread over all its queues (the margin: a difference below it is not established)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xB17C0DE
N = 10**9
K = 23
QUEUES = 5
HITS_CAP = 1 << 16


def timed_queue(torch, stream, fn, burst):
    """ms per call of one queue of `burst` back-to-back calls (no host wait inside), after one call of warm-up; fn(i) alternates its outputs with i"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    a.record(stream)
    for i in range(burst):
        fn(i + 1)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def spread(ms):
    return (max(ms) - min(ms)) / statistics.median(ms)


def word_of(codes):
    return int(sum(int(c) << (2 * i) for i, c in enumerate(codes)))


def fold(doc, parents):
    """the exact forms, tree against tree: this tree's median over the parent's, beside the parent's spread over all its queues"""
    doc["parent_libraries"] = [p["library"] for p in parents]
    doc["exact_vs_parent"] = []
    for run in doc["runs"]:
        theirs = [x for p in parents for r in p["runs"] if (r["family"], r["form"], r["n_queries"]) == (run["family"], run["form"], run["n_queries"])
                  for x in r["exact_ms"]]
        if not theirs:
            continue
        pm = statistics.median(theirs)
        doc["exact_vs_parent"].append({"family": run["family"], "form": run["form"], "n_queries": run["n_queries"], "parent_ms": theirs,
                                       "parent_median_ms": round(pm, 4), "parent_spread": round(spread(theirs), 4), "this_ms": run["exact_ms"],
                                       "this_median_ms": run["exact_median_ms"], "this_over_parent": round(run["exact_median_ms"] / pm, 4),
                                       "within_parent_spread": bool(run["exact_median_ms"] / pm - 1 <= spread(theirs))})
    doc["exact_forms_within_parent_spread"] = all(r["within_parent_spread"] for r in doc["exact_vs_parent"])
    return doc


def write(doc, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--qs", default="1,64,512")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the tree whose bitnuc_amd package (and built library) is measured")
    ap.add_argument("--parent", action="append", default=[], help="a document written with --exact-only --tree <the parent commit>")
    ap.add_argument("--fold", default=None, help="a document of this tree to fold the --parent documents into, without measuring")
    args = ap.parse_args()
    if args.fold:
        write(fold(json.load(open(args.fold)), [json.load(open(p)) for p in args.parent]), args.out)
        return
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import _lib as L, build
    assert os.path.abspath(os.path.dirname(os.path.dirname(bn.__file__))) == os.path.abspath(args.tree), bn.__file__
    build.ensure_built(build=False)
    n = args.n
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = bn.Context(0, stream=stream.cuda_stream)  # one stream: torch's buffer work and the timing events are ordered with the launches
    nw = (n + 31) // 32
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.nucgen_dev(ref, n, SEED)
    words = torch.zeros(nw, dtype=torch.int64, device=dev)
    ctx.encode_dev(ref, n, words)
    ctx.sync()
    rng = np.random.default_rng(2028)
    doc = {"tool": "tools/bench_kmer_pattern.py", "n_bases": n, "k": K, "seed": SEED, "queues": QUEUES, "device": torch.cuda.get_device_name(0),
           "library": L.load().bitnuc_version().decode(), "exact_only": bool(args.exact_only), "runs": []}

    def u64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)

    def u32(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint32)).reshape(-1).view(np.int32).copy()).to(dev)

    for nq in [int(x) for x in args.qs.split(",")]:
        guides = []
        for p in rng.integers(0, n - K, size=(nq + 1) // 2):
            h = ref[int(p):int(p) + 20].cpu().numpy()
            guides.append([int(((b >> 1) ^ (b >> 2)) & 3) for b in h])
        guides += [[int(c) for c in g] for g in rng.integers(0, 4, size=(nq // 2, 20))]
        queries = np.array([word_of(g + [0, 2, 2]) for g in guides], dtype=np.uint64)  # guide + AGG
        taus = np.array([(0, 3, 8, K)[i % 4] for i in range(nq)], dtype=np.uint32)
        dq, dt = u64(queries), u32(taus)
        out = {name: torch.zeros((2, nq), dtype=torch.int64, device=dev) for name in ("pc", "ec", "pp", "ep")}
        outd = {name: torch.zeros((2, nq), dtype=torch.uint8, device=dev) for name in ("pd", "ed")}
        hp = torch.zeros((2, 2, HITS_CAP), dtype=torch.int64, device=dev)
        hd = torch.zeros((2, 2, HITS_CAP), dtype=torch.uint8, device=dev)
        nh = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        q0 = int(queries[0])
        exact = {
            ("count_multi", "ascii"): lambda i: ctx.kmer_hdist_count_multi_dev(ref, n, K, dq, dt, nq, out["ec"][i & 1]),
            ("count_multi", "packed"): lambda i: ctx.kmer_hdist_count_multi_packed_dev(words, nw, n, K, dq, dt, nq, out["ec"][i & 1]),
            ("best", "ascii"): lambda i: ctx.kmer_hdist_best_async(ref, n, K, dq, nq, out["ep"][i & 1], outd["ed"][i & 1]),
            ("best", "packed"): lambda i: ctx.kmer_hdist_best_packed_async(words, nw, n, K, dq, nq, out["ep"][i & 1], outd["ed"][i & 1]),
        }
        if nq == 1:
            exact[("hits", "ascii")] = lambda i: ctx.kmer_hdist_hits_dev(ref, n, K, q0, 3, hp[1, i & 1], hd[1, i & 1], HITS_CAP, nh[1, (i & 1):])
            exact[("hits", "packed")] = lambda i: ctx.kmer_hdist_hits_packed_dev(words, nw, n, K, q0, 3, hp[1, i & 1], hd[1, i & 1], HITS_CAP, nh[1, (i & 1):])
        pattern, equal = {}, None
        if not args.exact_only:
            pam = np.stack([bn.pattern_from_iupac("".join("ACGT"[c] for c in g) + "NGG") for g in guides])
            single = np.stack([bn.pattern_from_2bit(int(q), K) for q in queries])
            dpat, dsingle = u32(pam), u32(single)
            use = {"p": dsingle, "h": single[0]}  # the singletons first (the equality check), then the PAM patterns (the timing)
            pattern = {
                ("count_multi", "ascii"): lambda i: ctx.kmer_pattern_count_multi_async(ref, n, K, use["p"], dt, nq, out["pc"][i & 1]),
                ("count_multi", "packed"): lambda i: ctx.kmer_pattern_count_multi_packed_async(words, nw, n, K, use["p"], dt, nq, out["pc"][i & 1]),
                ("best", "ascii"): lambda i: ctx.kmer_pattern_best_async(ref, n, K, use["p"], nq, out["pp"][i & 1], outd["pd"][i & 1]),
                ("best", "packed"): lambda i: ctx.kmer_pattern_best_packed_async(words, nw, n, K, use["p"], nq, out["pp"][i & 1], outd["pd"][i & 1]),
            }
            if nq == 1:
                pattern[("hits", "ascii")] = lambda i: ctx.kmer_pattern_hits_async(ref, n, K, use["h"], 3, hp[0, i & 1], hd[0, i & 1], HITS_CAP, nh[0, (i & 1):])
                pattern[("hits", "packed")] = lambda i: ctx.kmer_pattern_hits_packed_async(words, nw, n, K, use["h"], 3, hp[0, i & 1], hd[0, i & 1], HITS_CAP,
                                                                                          nh[0, (i & 1):])
            equal = {}
            for key in exact:  # singleton patterns must reproduce the exact entry points bit for bit
                pattern[key](0)
                exact[key](0)
                ctx.sync()
                if key[0] == "count_multi":
                    same = bool(torch.equal(out["pc"][0], out["ec"][0]))
                elif key[0] == "best":
                    same = bool(torch.equal(out["pp"][0], out["ep"][0])) and bool(torch.equal(outd["pd"][0], outd["ed"][0]))
                else:
                    m = min(int(nh[1, 0]), HITS_CAP)
                    same = int(nh[0, 0]) == int(nh[1, 0]) and bool(torch.equal(hp[0, 0, :m], hp[1, 0, :m])) and bool(torch.equal(hd[0, 0, :m], hd[1, 0, :m]))
                assert same, ("singleton patterns differ from the exact form", key, nq)
                equal["/".join(key)] = same
            use["p"], use["h"] = dpat, pam[0]
        burst = 8 if nq == 1 else (4 if nq <= 64 else 2)
        for key, efn in exact.items():
            pms, ems = [], []
            for _ in range(QUEUES):  # alternating: both forms see the same drift of the chip
                if pattern:
                    pms.append(timed_queue(torch, stream, pattern[key], burst))
                ems.append(timed_queue(torch, stream, efn, burst))
            ctx.sync()
            run = {"family": key[0], "form": key[1], "n_queries": nq, "burst": burst, "exact_ms": [round(x, 4) for x in ems],
                   "exact_median_ms": round(statistics.median(ems), 4), "exact_spread": round(spread(ems), 4)}
            if pattern:
                run.update({"pattern_ms": [round(x, 4) for x in pms], "pattern_median_ms": round(statistics.median(pms), 4),
                            "pattern_spread": round(spread(pms), 4), "pattern_over_exact": round(statistics.median(pms) / statistics.median(ems), 4),
                            "singletons_equal_exact": equal["/".join(key)]})
                if key[0] == "count_multi":
                    run["pattern_counts_head"] = out["pc"][burst & 1][:4].cpu().tolist()
                elif key[0] == "hits":
                    run["pattern_n_hits"] = int(nh[0, burst & 1])
            doc["runs"].append(run)
            print(json.dumps(run), flush=True)
    if not args.exact_only:
        doc["singletons_equal_exact_everywhere"] = all(r["singletons_equal_exact"] for r in doc["runs"])
    write(doc, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
