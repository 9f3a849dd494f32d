"""The plan of the argument sweep over the searches along a reference (tests/test_kmer_ref_args.py): the 56 entry points -- seven families (Hamming hit
list, count, best match, histogram; edit-distance best match, count, hit list) x exact queries / patterns x ASCII / packed x asynchronous / host --, one
valid base call each at the smallest shape that has every part, and every single argument fault and every pair of faults on different arguments.

What a call with bad arguments answers is decided by the ORDER of the checks in front of the launch, and a pair of faults is what shows an order: the
first check that fires names the status and err.value.  Per case the sweep records (status, err.value, err.index, err.byte, mask), mask bit i set while
output i still holds the sentinel.  The expected values are recorded results (tests/golden/kmer_ref_args.json), written by this module's main() from the
library as it stood BEFORE the host dispatch was rewritten (csrc/ref_dispatch.h), so they pin what callers saw, not what the code under test gives.

The host forms run through a NULL context below the host cutoff.  The asynchronous forms run on a device, so every case must be one the library either
refuses before any launch or defines as legal: a device pointer that is NULL or misaligned is refused by the checks (data, queries, taus and every output
but the distance bytes), d_ref, dist and hit_dist may have any alignment, hit_dist may be NULL, pos may be NULL with cap 0, and a pattern of a hit list
is a host pointer that the launchers read by value.  Every buffer carries SLACK bytes behind its payload, so a pointer advanced by up to 4 bytes stays
inside it."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys
from collections import namedtuple

import numpy as np

N, K, NQ, CAP, N_BINS, TAU, N_WORDS = 40, 5, 2, 4, 3, 1, 2
MAX_QUERIES, HIST_MAX_BINS = 65536, 16  # BITNUC_MAX_QUERIES, BITNUC_HIST_MAX_BINS (include/bitnuc_hip.h; tests/test_kmer_ref_args.py holds them against it)
SLACK = 64
SENTINEL = 0xA5
NULL = "NULL"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_ref_args.json")

Entry = namedtuple("Entry", "symbol family edist pattern packed host")
FAMILIES = (("hits", False), ("count", False), ("best", False), ("hist", False), ("best", True), ("count", True), ("hits", True))
# the arguments behind (ctx, data, [n_words,] n, k) and in front of err
ARGS = {"count": ("queries", "taus", "nq", "counts"), "best": ("queries", "nq", "pos", "dist"), "hist": ("queries", "nq", "n_bins", "hist"),
        "hits": ("query", "tau", "pos", "hit_dist", "cap", "n_hits")}
OUTPUTS = {"count": ("counts",), "best": ("pos", "dist"), "hist": ("hist",), "hits": ("pos", "hit_dist", "n_hits")}
POINTERS = ("data", "queries", "taus", "query", "counts", "pos", "dist", "hist", "hit_dist", "n_hits")


def _symbol(family, edist, pattern, packed, host):
    stem = {"count": "count_multi", "best": "best", "hist": "hist", "hits": "hits"}[family]
    kind = ("pattern_edist" if pattern else "edist") if edist else ("pattern" if pattern else "hdist")
    dev = "_dev" if kind == "hdist" and family in ("count", "hits") else "_async"  # the two oldest families' device forms predate the _async suffix
    return f"bitnuc_kmer_{kind}_{stem}" + ("_packed" if packed else "") + ("" if host else dev)


ENTRIES = tuple(Entry(_symbol(f, e, p, w, h), f, e, p, w, h)
                for (f, e), p, w, h in itertools.product(FAMILIES, (False, True), (False, True), (False, True)))


def arg_names(entry):
    return ("data",) + (("n_words",) if entry.packed else ()) + ("n", "k") + ARGS[entry.family]


def pointers(entry):
    """the pointer arguments of an entry point, in argument order (an exact hit list takes its query by value)"""
    return tuple(a for a in arg_names(entry) if a in POINTERS and not (a == "query" and not entry.pattern))


def aligned8(entry, name):
    """the pointer arguments that are arrays of 8-byte words"""
    return name in ("counts", "pos", "hist", "n_hits") or (name == "data" and entry.packed) or (name == "queries" and not entry.pattern)


def faults(entry):
    """[(label, {argument: value, NULL or ("+", bytes)})]: the single faults that apply to this entry point"""
    f = [("k=0", {"k": 0}), ("k=33", {"k": 33}), ("n=k-1", {"n": K - 1})]
    if entry.packed:
        f.append(("n_words-1", {"n_words": N_WORDS - 1}))
    if "nq" in ARGS[entry.family]:
        f += [("nq=0", {"nq": 0}), ("nq>max", {"nq": MAX_QUERIES + 1})]
    if entry.family == "hist":
        f += [("bins=0", {"n_bins": 0}), ("bins>max", {"n_bins": HIST_MAX_BINS + 1})]
    if entry.family == "hits":
        f.append(("cap=0,pos=NULL", {"cap": 0, "pos": NULL}))
    for p in pointers(entry):
        f += [(p + "=NULL", {p: NULL}), (p + "+1", {p: ("+", 1)})]
        if aligned8(entry, p):
            f.append((p + "+4", {p: ("+", 4)}))
    return f


def cases(entry):
    """[(label, overrides)]: the base call, every single fault, every pair of faults on different arguments"""
    f = faults(entry)
    out = [("base", {})] + f
    for (la, a), (lb, b) in itertools.combinations(f, 2):
        if not set(a) & set(b):
            out.append((la + " & " + lb, {**a, **b}))
    return out


def labels_digest(entry):
    return hashlib.sha1("\n".join(label for label, _ in cases(entry)).encode()).hexdigest()[:12]


# ---- the buffers -----------------------------------------------------------------------------------------------------------
def _payloads(entry):
    """name -> (bytes of the payload, the byte its slack holds); outputs have no payload and are sentinel throughout"""
    rng = np.random.default_rng(0x5EED)
    codes = rng.integers(0, 4, size=N)
    queries = rng.integers(0, 2**62, size=NQ, dtype=np.uint64)
    if entry.packed:
        words = np.zeros(N_WORDS, dtype=np.uint64)
        for i, c in enumerate(codes):
            words[i // 32] |= np.uint64(int(c) << (2 * (i % 32)))
        data = (words.view(np.uint8), 0)
    else:
        data = (np.frombuffer(b"ACGT", dtype=np.uint8)[codes], ord("A"))  # a pointer advanced by a byte still reads bases
    pats = np.zeros((NQ, 4), dtype=np.uint32)
    for q in range(NQ):
        for i in range(K):
            pats[q, (int(queries[q]) >> (2 * i)) & 3] |= 1 << i
        pats[q, 0] |= 1 << (K - 1)  # the last position also takes an A
    p = {"data": data, "queries": ((pats if entry.pattern else queries).view(np.uint8).reshape(-1), 0),
         "taus": (np.full(NQ, TAU, dtype=np.uint32).view(np.uint8), 0), "query": (pats[0].view(np.uint8), 0)}
    return p, int(queries[0])


OUT_BYTES = {"counts": NQ * 8, "pos": max(NQ, CAP) * 8, "dist": NQ, "hist": NQ * N_BINS * 8, "hit_dist": CAP, "n_hits": 8}


class HostMem:
    """64-byte aligned host buffers"""

    def __init__(self):
        self.bufs = {}

    def alloc(self, name, content):
        raw = np.empty(content.size + 64, dtype=np.uint8)
        off = (-raw.ctypes.data) % 64
        self.bufs[name] = (raw, raw[off:off + content.size])
        self.bufs[name][1][:] = content
        return self.bufs[name][1].ctypes.data

    def refill(self, names):
        for n in names:
            self.bufs[n][1][:] = SENTINEL

    def intact(self, name):
        return bool((self.bufs[name][1] == SENTINEL).all())

    def settle(self):
        pass


class DevMem:
    """device buffers (torch: at least 256-byte aligned); settle() orders torch's stream in front of the context's"""

    def __init__(self):
        import torch
        self.torch = torch
        self.bufs = {}

    def alloc(self, name, content):
        self.bufs[name] = self.torch.from_numpy(np.ascontiguousarray(content).copy()).to("cuda:0")
        assert self.bufs[name].data_ptr() % 64 == 0
        return self.bufs[name].data_ptr()

    def refill(self, names):
        for n in names:
            self.bufs[n].fill_(SENTINEL)

    def intact(self, name):
        return bool((self.bufs[name] == SENTINEL).all().item())

    def settle(self):
        self.torch.cuda.synchronize()


def run(entry, lib, ctx_handle=None):
    """every case of the entry point, in cases() order -> [(status, err.value, err.index, err.byte, mask)].  ctx_handle: the context of the asynchronous
    forms (a c_void_p); the host forms take a NULL context."""
    from bitnuc_amd import _lib as L
    assert entry.host == (ctx_handle is None)
    fn = getattr(lib, entry.symbol)
    payloads, query = _payloads(entry)
    host, mem = HostMem(), (HostMem() if entry.host else DevMem())
    outs = OUTPUTS[entry.family]
    addr = {}
    for name in pointers(entry):
        if name in outs:
            addr[name] = mem.alloc(name, np.full(OUT_BYTES[name] + SLACK, SENTINEL, dtype=np.uint8))
        else:
            content, slack = payloads[name]
            where = host if name == "query" else mem  # a hit list's pattern is a host pointer in every form
            addr[name] = where.alloc(name, np.concatenate([content, np.full(SLACK, slack, dtype=np.uint8)]))
    names = arg_names(entry)
    sig = L.SIGNATURES[entry.symbol][1]
    assert len(sig) == len(names) + 2
    results = []
    dirty = ()
    for label, over in cases(entry):
        mem.refill(dirty)
        mem.settle()
        v = {"n": N, "k": K, "n_words": N_WORDS, "nq": NQ, "n_bins": N_BINS, "tau": TAU, "cap": CAP, "query": query}
        v.update(addr)
        for a, o in over.items():
            v[a] = 0 if o == NULL else v[a] + o[1] if isinstance(o, tuple) else o
        args = []
        for a, t in zip(names, sig[1:-1]):
            if a in addr:
                p = C.c_void_p(v[a] or None)
                args.append(p if t is C.c_void_p else C.cast(p, t))
            else:
                args.append(v[a])
        err = L.BitnucErr()
        st = fn(ctx_handle, *args, C.byref(err))
        if ctx_handle is not None:
            e2 = L.BitnucErr()
            assert lib.bitnuc_ctx_sync(ctx_handle, C.byref(e2)) == L.OK, (entry.symbol, label, e2.status, e2.backend_code)
        assert st == err.status, (entry.symbol, label)
        dirty = tuple(o for o in outs if not mem.intact(o))
        mask = sum(1 << i for i, o in enumerate(outs) if o not in dirty)
        results.append((int(st), int(err.value), int(err.index), int(err.byte), mask))
    return results


# ---- the fixture: per symbol the distinct results and one letter per case ---------------------------------------------------
LETTERS = "0123456789abcdefghijklmnopqrstuvwxyz"


def pack(entry, results):
    uniq = sorted(set(results))
    assert len(uniq) <= len(LETTERS)
    return {"labels": labels_digest(entry), "results": [list(u) for u in uniq], "cases": "".join(LETTERS[uniq.index(r)] for r in results)}


def unpack(rec):
    return [tuple(rec["results"][LETTERS.index(ch)]) for ch in rec["cases"]]


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main(argv):
    """python tests/kmer_ref_args.py host|async OUT.json [MERGE.json]: record the half's results (merged into MERGE.json's other half)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bitnuc_amd import _lib as L, build
    build.ensure_built()
    lib = L.load()
    half, out = argv[1], argv[2]
    fixture = json.load(open(argv[3])) if len(argv) > 3 else {}
    ctx = None
    if half == "async":
        import bitnuc_amd
        ctx = bitnuc_amd.Context(0)
    for e in ENTRIES:
        if e.host == (half == "host"):
            fixture[e.symbol] = pack(e, run(e, lib, None if e.host else ctx._h))
    with open(out, "w") as f:
        json.dump(fixture, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(half, sum(len(fixture[e.symbol]["cases"]) for e in ENTRIES if e.host == (half == "host")), "cases")


if __name__ == "__main__":
    main(sys.argv)
