"""The plan of the asynchronous-queue tests (tests/test_gpu_queue.py): the operation kinds, their order, sizes and buffers, the planted errors, and a
host model that walks a queue with the oracle and numpy alone (no GPU; tests/test_queue_plan.py checks the plan).

A pipeline queues many _dev calls on a context and syncs once.  What differs from N single calls is what a context carries from one launch to the next:
the accumulators and tickets of the single-launch reductions (d_acc / d_tickets, "zero between launches"), the scratch slots several families share
(ensure_scratch), and the ring of error slots.  The plan puts EVERY ordered pair of kinds next to each other once: an Eulerian circuit of the complete
directed graph on the kinds, self-loops included, cut into queues that overlap by one operation.

Queue length: the issue allows 64.  The errors ask for every ASCII kind once as the earlier (i) and once as the later (j) of two failing operations, one pair
per queue, in about a third of the queues: 14 ASCII kinds need 14 such queues, so the circuit's 841 edges are cut into 39 queues of at most 23 operations.

Buffers.  Three shared ones carry data by stream order alone: `seq` (ASCII, written by nucgen), `words` (written by encode_dev), `seq2` (ASCII, written by
decode_dev).  Packed consumers read `words` as the latest producer left it; ASCII consumers read `seq2` when a decode is the latest of the two ASCII
producers, `seq` otherwise.  Every other output is private to its operation and pre-filled with 0xA5 (guards included); the 8-byte result cells of the
counts, n_hits and hdist sit next to each other in one array `cells` (operation p owns cells[p + 1]).  The model never calls the product."""
from collections import namedtuple

import numpy as np

import alphabet

Kind = namedtuple("Kind", "name symbol reads host")  # reads: "ascii", "packed" or None; host: a synchronous host-pointer call through the context

KINDS = (
    Kind("nucgen", "bitnuc_nucgen_dev", None, False),
    Kind("encode", "bitnuc_encode_dev", "ascii", False),
    Kind("decode", "bitnuc_decode_dev", "packed", False),
    Kind("encode_tables", "bitnuc_encode_batch_dev", "ascii", False),        # scratch 6 (pad plan) and 7 (tile_base)
    Kind("decode_tables", "bitnuc_decode_batch_dev", "packed", False),
    Kind("encode_plan", "bitnuc_encode_batch_plan_dev", "ascii", False),
    Kind("decode_plan", "bitnuc_decode_batch_plan_dev", "packed", False),
    Kind("encode_fixed", "bitnuc_encode_fixed_dev", "ascii", False),         # back to back
    Kind("decode_fixed_gap", "bitnuc_decode_fixed_dev", "packed", False),    # stride = read_len + 3
    Kind("kmers_dense", "bitnuc_as_2bit_batch_dev", "ascii", False),         # stride = k
    Kind("kmers_windows", "bitnuc_as_2bit_batch_dev", "ascii", False),       # stride = 1
    Kind("scan", "bitnuc_kmer_hdist_scan_dev", "ascii", False),
    Kind("count_aligned", "bitnuc_kmer_hdist_count_dev", "ascii", False),    # kmer_count3_mfma_kernel: d_acc[5], d_tickets[2]
    Kind("count_at7", "bitnuc_kmer_hdist_count_dev", "ascii", False),        # ref + 7: kmer_scan2_kernel, the same accumulator and ticket, another grid
    Kind("scan_packed", "bitnuc_kmer_hdist_scan_packed_dev", "packed", False),
    Kind("count_packed", "bitnuc_kmer_hdist_count_packed_dev", "packed", False),  # d_acc[6], d_tickets[3]
    Kind("hits", "bitnuc_kmer_hdist_hits_dev", "ascii", False),              # scratch 7, three launches on one slot
    Kind("hits_cap0", "bitnuc_kmer_hdist_hits_dev", "ascii", False),         # cap = 0: no emit pass
    Kind("hits_packed", "bitnuc_kmer_hdist_hits_packed_dev", "packed", False),
    Kind("multi", "bitnuc_kmer_hdist_count_multi_dev", "ascii", False),      # scratch 8, one latch per call
    Kind("multi_packed", "bitnuc_kmer_hdist_count_multi_packed_dev", "packed", False),
    Kind("hdist", "bitnuc_hdist_dev", "packed", False),                      # d_acc[4], d_tickets[1]
    Kind("base_counts", "bitnuc_base_counts_dev", "packed", False),          # d_acc[0..2], d_tickets[0]
    Kind("hdist_pairs", "bitnuc_hdist_pairs_dev", "packed", False),
    Kind("hdist_query", "bitnuc_hdist_query_dev", "packed", False),
    Kind("split", "bitnuc_split_packed_dev", "packed", False),
    Kind("host_encode", "bitnuc_encode", "ascii", True),                     # flush_pending + staging scratch
    Kind("host_hits", "bitnuc_kmer_hdist_hits", "ascii", True),              # scratch 0-3 and 7
    Kind("host_multi_packed", "bitnuc_kmer_hdist_count_multi_packed", "packed", True),  # scratch 0-2 and 8
)
NAMES = tuple(k.name for k in KINDS)
KIND = {k.name: k for k in KINDS}
ASCII_KINDS = tuple(k.name for k in KINDS if k.reads == "ascii")
HOST_KINDS = tuple(k.name for k in KINDS if k.host)
# the _dev symbols of include/bitnuc_hip.h that are NOT operation kinds, and why
EXCLUDED_DEV_SYMBOLS = {
    "bitnuc_batch_word_offsets_dev": "synchronous table builder (returns total_words to the host)",
    "bitnuc_batch_plan_build_dev": "synchronous table builder (the plans are built before the queue starts)",
    "bitnuc_batch_plan_word_offsets_dev": "accessor of a plan's table, no launch",
    "bitnuc_allgather_words_dev": "comm (RCCL; tests/test_gpu_comm.py)",
    "bitnuc_allgatherv_words_dev": "comm",
    "bitnuc_encode_sharded_allgather_dev": "comm",
    "bitnuc_encode_sharded_allgather_overlapped_dev": "comm",
    "bitnuc_stream_probe_dev": "probe: a bandwidth measurement, no result to compare",
}

MAX_QUEUE = 23
FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
CAP = 300_032          # bytes of seq / seq2 that hold bases (a multiple of 32; the largest size + the 7-byte offset of count_at7 fit)
NW = 12_000           # words of `words` / `words_b`: CAP / 32 and the ragged layout's padded words fit
GUARD = 64             # 0xA5 bytes after each shared buffer
AT7 = 7

# the constants the sizes rest on (tests/test_queue_plan.py reads them back from the sources' text)
K_BLOCK, COUNT_ROUNDS, HITS_ROUNDS, HITS_TILE, MULTI_QB, BATCH_TILE = 256, 4, 4, 4096, 16, 64
SLOT_PAD_PLAN, SLOT_TILES, SLOT_MULTI = 6, 7, 8  # ensure_scratch's `which`: the batch's pad plan; hit lists' counts + tile offsets AND the batch's tile_base; the multi-query tables
TABLE_BYTES = 64 * 12 * 4 + 16                   # sizeof(Count3MfmaTable)
COUNT_WG_WINDOWS = (K_BLOCK // 64) * COUNT_ROUNDS * 1024  # windows a count workgroup covers per pass

KS = (1, 16, 21, 31, 32)
# n < k (no windows: the memset path, no ticket), tail windows only, then 4 ... 18 count workgroups (70 001 ... 299 983 bases)
N_KMER = ("lt", "k5", 70_001, 131_077, 200_003, 299_983)
N_QUERIES = (1, 16, 17)
READS = (150, 1500)    # read length, count: the fixed layout of the ragged-batch kinds


def scan_rounds(n, skip=0):
    return alphabet.scan_rounds(n, skip)


def hits_trips(n, skip=0):
    """per-trip counts of a hit list: the trips, the head's and the tail's (kmer.hip launch_hits)"""
    return (scan_rounds(n, skip) + HITS_ROUNDS - 1) // HITS_ROUNDS + 2


def hits_scratch_bytes(ntr):
    """kmer.hip hits_scratch: the counts padded to 256 bytes, then one u64 per tile"""
    return ((4 * ntr + 255) & ~255) + 8 * ((ntr + HITS_TILE - 1) // HITS_TILE)


def batch_scratch_bytes(total_words):
    """batch.hip: (slot 6 pad plan, slot 7 tile_base) of a table-driven batch"""
    ntiles = (total_words + BATCH_TILE - 1) // BATCH_TILE
    return total_words + 2 + BATCH_TILE, (ntiles + 1 + 2) * 8


def multi_scratch_bytes(nq):
    return nq * TABLE_BYTES


def scratch_capacity(old_cap, nbytes):
    """runtime.hip ensure_scratch: unchanged when it fits, else max(bytes, 1.5 x old) rounded up to 4 KiB"""
    if nbytes <= old_cap:
        return old_cap
    return (max(nbytes, old_cap + old_cap // 2) + 4095) & ~4095


# ---- order ---------------------------------------------------------------------------------------------------------------------
def euler_circuit(n):
    """Hierholzer on the complete directed graph on n vertices with self-loops, from vertex 0, every vertex's edges taken in the fixed order
    v + 1, v + 2, ... (mod n), the self-loop last -> n * n + 1 vertices, first == last; every ordered pair adjacent exactly once."""
    nxt = [0] * n
    order = [[(v + 1 + d) % n for d in range(n)] for v in range(n)]
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(order[v][nxt[v]])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


def cut(circuit, length=MAX_QUEUE):
    """queues of at most `length` vertices; each starts with the last vertex of the one before, so no adjacency is lost at a cut"""
    out, s = [], 0
    while s < len(circuit) - 1:
        out.append((s, circuit[s:s + length]))
        s += length - 1
    return out


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
def _mix(x):
    """splitmix64's finaliser: the plan's only source of 'arbitrary' numbers"""
    x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return x ^ (x >> 31)


def _taus(k):
    return (0, 1, 3 * k // 4, k)


def ragged_lengths():
    """about 3000 sequences: empties, one-base reads, lengths around the word and tile sizes, a few long ones"""
    out = []
    for i in range(3001):
        r = _mix(i) % 100
        out.append(0 if r < 12 else 1 if r < 16 else (31, 32, 33, 64, 65, 95)[i % 6] if r < 22 else (2047, 2049)[i % 2] if r == 22
                   else 5003 if i % 500 == 250 else 1 + _mix(i + 77) % 150)
    return out


def layouts():
    """name -> (offsets int64[count + 1], word offsets int64[count + 1]): 150-base reads from byte 0, and the ragged mix from byte 7"""
    L, count = READS
    reads = np.arange(count + 1, dtype=np.int64) * L
    lens = np.array(ragged_lengths(), dtype=np.int64)
    rag = np.concatenate([[0], np.cumsum(lens)]) + AT7
    out = {}
    for name, off in (("reads", reads), ("ragged", rag)):
        wo = np.concatenate([[0], np.cumsum((np.diff(off) + 31) // 32)]).astype(np.int64)
        assert off[-1] <= CAP and wo[-1] <= NW
        out[name] = (off, wo)
    return out


Op = namedtuple("Op", "pos kind p")  # pos: index in the circuit; p: the parameters (dict)


def params(kind, r):
    """the parameters of the r-th occurrence of `kind` in the circuit (rotating through the kind's table)"""
    ki = NAMES.index(kind)
    r = r + 7 * ki
    k = KS[r % 5]
    nsel = N_KMER[r % 6]
    p = {"seed": _mix(1000 * ki + r) >> 1}
    kmer = {"k": k, "n": k - 1 if nsel == "lt" else k + 5 if nsel == "k5" else nsel, "tau": _taus(k)[(r // 2) % 4], "query": _mix(p["seed"])}
    if kind == "nucgen":
        p.update(n=(5, 1000, 70_001, 299_983, CAP)[r % 5], flags=(0, 2, 0, 1)[r % 4])
    elif kind in ("encode", "decode", "host_encode"):
        p.update(n=(1, 31, 33, 4097, 70_001, 131_077, 299_983)[r % 7] if not KIND[kind].host else (4097, 70_001, 131_077)[r % 3])
    elif kind in ("encode_tables", "decode_tables", "encode_plan", "decode_plan"):
        p.update(layout=("reads", "ragged")[r % 2])
    elif kind in ("encode_fixed", "decode_fixed_gap"):
        L, count = ((150, 1500), (33, 4001), (100, 2003))[r % 3]
        p.update(L=L, count=count, stride=L + 3 if kind == "decode_fixed_gap" else L)
    elif kind == "kmers_dense":
        n = (k + 5, 70_001, 299_983)[r % 3]
        p.update(k=k, stride=k, count=n // k)
    elif kind == "kmers_windows":
        n = (k + 5, 70_001, 131_077)[r % 3]
        p.update(k=k, stride=1, count=n - k + 1)
    elif kind in ("scan", "count_aligned", "count_at7", "scan_packed", "count_packed", "hits_cap0"):
        p.update(kmer)
    elif kind in ("hits", "hits_packed", "host_hits"):
        p.update(kmer, cap=(5000, 4097, 300_000)[r % 3])
        if kind == "host_hits" and p["n"] > 200_000:
            p["n"] = 70_001
    elif kind in ("multi", "multi_packed", "host_multi_packed"):
        nq = N_QUERIES[(r // 2) % 3] if kind != "host_multi_packed" else (1, 17)[r % 2]
        high = ~((1 << (2 * k)) - 1) & (2**64 - 1)
        qs = [kmer["query"]] + [_mix(kmer["query"] + j) for j in range(1, nq)]
        if nq > 1:  # one query repeated under different high bits
            qs[1] = (qs[0] & ~high) | (~qs[0] & high)
        p.update(kmer, nq=nq, queries=qs, taus=[_taus(k)[(j + r) % 4] for j in range(nq)])
        if kind == "host_multi_packed" and p["n"] > 200_000:
            p["n"] = 131_077
    elif kind in ("hdist", "base_counts"):
        p.update(n=(1, 33, 70_001, 299_983)[r % 4])
    elif kind in ("hdist_pairs", "hdist_query"):
        p.update(count=(1, 255, 256, 4099, NW)[r % 5], len=KS[(r // 5) % 5], query=_mix(p["seed"] + 1))
    elif kind == "split":
        slen = (33, 70_001, 299_983)[r % 3]
        p.update(slen=slen, idx=(0, 5, slen // 2 + 5, slen)[(r // 3) % 4])
    else:
        raise KeyError(kind)
    return p


def examined(op, lay=None):
    """the byte range [lo, hi) of the call's ASCII input in which an invalid byte is found (relative to the pointer the call is given); hi == lo: none"""
    k, p = op.kind, op.p
    if KIND[k].reads != "ascii":
        return 0, 0
    if k in ("encode", "host_encode"):
        return 0, p["n"]
    if k in ("encode_tables", "encode_plan"):
        off = (lay or layouts())[p["layout"]][0]
        return int(off[0]), int(off[-1])
    if k == "encode_fixed":
        return 0, p["count"] * p["L"]
    if k == "kmers_dense":
        return 0, p["count"] * p["k"]
    if k == "kmers_windows":
        return 0, p["count"] + p["k"] - 1
    return (0, p["n"]) if p["n"] >= p["k"] else (0, 0)


def takes_slot(op):
    """an asynchronous launch that owns an error slot (what a capture counts)"""
    lo, hi = examined(op)
    return not KIND[op.kind].host and hi > lo


Queue = namedtuple("Queue", "index ops errors")  # errors: {position in the queue: (byte, index)}


def build_plan():
    """-> list of Queue"""
    circ = euler_circuit(len(KINDS))
    seen = {}
    ops = []
    for t, v in enumerate(circ):
        kind = NAMES[v]
        r = seen.get(kind, 0)
        seen[kind] = r + 1
        ops.append(Op(t, kind, params(kind, r)))
    lay = layouts()
    queues = [[s, ops[s:s + MAX_QUEUE], {}] for s, _ in cut(circ)]
    # errors: ASCII kind t as the earlier and kind t + 5 as the later of two failing operations, each pair in the first queue (walking from a start that
    # spreads them over the circuit) that has both with bytes to examine, in that order
    A = len(ASCII_KINDS)
    used = set()
    for t in range(A):
        ki, kj = ASCII_KINDS[t], ASCII_KINDS[(t + 5) % A]
        start = (t * len(queues)) // A
        for d in range(len(queues)):
            q = (start + d) % len(queues)
            if q in used:
                continue
            qops = queues[q][1]
            ii = [x for x, o in enumerate(qops) if o.kind == ki and examined(o, lay)[1] > examined(o, lay)[0]]
            jj = [x for x, o in enumerate(qops) if o.kind == kj and examined(o, lay)[1] > examined(o, lay)[0]]
            pair = [(i, j) for i in ii for j in jj if i < j]
            if not pair:
                continue
            i, j = pair[0]
            bi = alphabet.INVALID_VALID_SELECTOR[_mix(t) % len(alphabet.INVALID_VALID_SELECTOR)] if t % 2 == 0 else alphabet.INVALID_OTHER[_mix(t) % len(alphabet.INVALID_OTHER)]
            bj = alphabet.other_class(bi, t)
            for x, b in ((i, bi), (j, bj)):
                lo, hi = examined(qops[x], lay)
                queues[q][2][x] = (b, lo + _mix(31 * t + x) % (hi - lo))
            used.add(q)
            break
        else:
            raise AssertionError(("no queue holds", ki, "before", kj))
    return [Queue(n, q[1], q[2]) for n, q in enumerate(queues)]


_PLAN = None


def plan():
    global _PLAN
    if _PLAN is None:
        _PLAN = build_plan()
    return _PLAN


# ---- the host model ---------------------------------------------------------------------------------------------------------------
def initial_buffers(oracle, salt=0):
    """the shared buffers as uploaded before a queue starts: valid bases everywhere (any prefix is a valid input), arbitrary words; salt: other data"""
    g = np.full(GUARD, FILL, np.uint8)
    rng = np.random.default_rng(0xB17 + salt)
    return {"seq": np.concatenate([oracle.nucgen(CAP, 101 + salt, 0, 2), g]), "seq2": np.concatenate([oracle.nucgen(CAP, 202 + salt), g]),
            "words": np.concatenate([rng.integers(0, 2**64, NW, dtype=np.uint64), np.full(8, FILL64, np.uint64)]),
            "words_b": rng.integers(0, 2**64, NW, dtype=np.uint64)}


def _mask(q, k):
    return q & ((1 << (2 * k)) - 1)


def _fill(n, dtype=np.uint8):
    return np.full(n, FILL if dtype == np.uint8 else FILL64, dtype)


def _put(n_guarded, values, dtype):
    out = _fill(n_guarded, dtype)
    out[:len(values)] = values
    return out


def _batch_encode(oracle, s, off):
    parts = [oracle.encode(s[int(a):int(b)]) for a, b in zip(off[:-1], off[1:]) if b > a]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


Step = namedtuple("Step", "op src inputs outs cell unspecified raises host_result")
# src: the ASCII buffer read ("seq" / "seq2") or None; inputs: private arrays uploaded before the queue (bad copies, queries, taus, host inputs);
# outs: name -> the whole private output buffer as expected (guards and untouched bytes 0xA5): its size and dtype are the allocation;
# cell: the expected cells[p + 1] (u64) or None; unspecified: outputs not compared (an error operation); raises: (byte, index) a host call raises at once;
# host_result: name -> array a host call returns


def model(queue, oracle, lay=None, salt=0):
    """Walk the queue -> (steps, final shared buffers, the (byte, index) reports of the syncs after the queue, in order; then one clean sync)"""
    lay = lay or layouts()
    buf = initial_buffers(oracle, salt)
    ascii_src = "seq"
    steps = []
    pending, deferred = [], []  # errors latched since the last drain; errors implicit drains found (include/bitnuc_hip.h: a FIFO)
    for x, op in enumerate(queue.ops):
        k, p = op.kind, op.p
        kd = KIND[k]
        err = queue.errors.get(x)
        src = ascii_src if kd.reads == "ascii" else None
        s = buf[src][:CAP] if src else None
        w = buf["words"][:NW]
        inputs, outs, cell, raises, host_result = {}, {}, None, None, {}
        if err is not None:
            bad = buf[src].copy()
            bad[(AT7 if k == "count_at7" else 0) + err[1]] = err[0]
            inputs["bad"] = bad
        if kd.host:  # flush_pending: an implicit drain defers the first latched error
            if pending:
                deferred.append(pending[0])
            pending = []
            if err is not None:
                raises = err
        elif err is not None:
            pending.append(err)
        if k == "nucgen":
            buf["seq"][:p["n"]] = oracle.nucgen(p["n"], p["seed"], 0, p["flags"])
            ascii_src = "seq"
        elif k == "encode":
            e = oracle.encode(s[:p["n"]])
            if err is None:
                buf["words"][:len(e)] = e
            else:  # an error operation's output is unspecified: it gets a private one, `words` stays as it was
                outs["words"] = _put(len(e) + 2, e, np.uint64)
        elif k == "decode":
            buf["seq2"][:p["n"]] = oracle.decode(w[:(p["n"] + 31) // 32], p["n"])
            ascii_src = "seq2"
        elif k in ("encode_tables", "encode_plan"):
            off, wo = lay[p["layout"]]
            outs["words"] = _put(int(wo[-1]) + 2, _batch_encode(oracle, s, off), np.uint64)
        elif k in ("decode_tables", "decode_plan"):
            off, wo = lay[p["layout"]]
            out = _fill(int(off[-1]) + GUARD)
            for a, b, c in zip(off[:-1], off[1:], wo[:-1]):
                if b > a:
                    out[a:b] = oracle.decode(w[c:c + (b - a + 31) // 32], int(b - a))
            outs["back"] = out
        elif k == "encode_fixed":
            L, count = p["L"], p["count"]
            outs["words"] = _put(count * ((L + 31) // 32) + 2, np.concatenate([oracle.encode(s[r * L:(r + 1) * L]) for r in range(count)]), np.uint64)
        elif k == "decode_fixed_gap":
            L, count, stride, wpr = p["L"], p["count"], p["stride"], (p["L"] + 31) // 32
            out = _fill((count - 1) * stride + L + GUARD)
            for r in range(count):
                out[r * stride:r * stride + L] = oracle.decode(w[r * wpr:(r + 1) * wpr], L)
            outs["back"] = out
        elif k in ("kmers_dense", "kmers_windows"):
            outs["kmers"] = _put(p["count"] + 2, oracle.as_2bit_batch(s, p["k"], p["stride"], p["count"]), np.uint64)
        elif k == "hdist":
            nw = (p["n"] + 31) // 32
            cell = (FILL64 & ~0xFFFFFFFF) | oracle.hdist(w[:nw], buf["words_b"][:nw], p["n"])
        elif k == "base_counts":
            outs["counts"] = _put(6, np.array(oracle.base_counts(w[:(p["n"] + 31) // 32], p["n"]), np.uint64), np.uint64)
        elif k == "hdist_pairs":
            outs["dist"] = _put(p["count"] + GUARD, oracle.hdist_pairs(w[:p["count"]], buf["words_b"][:p["count"]], p["len"]), np.uint8)
        elif k == "hdist_query":
            outs["dist"] = _put(p["count"] + GUARD, oracle.hdist_pairs(np.full(p["count"], p["query"], np.uint64), w[:p["count"]], p["len"]), np.uint8)
        elif k == "split":
            nw = (p["slen"] + 31) // 32
            lo, ro = oracle.split_packed(w[:nw], p["slen"], p["idx"])
            outs["left"], outs["right"] = _put(nw + 3, lo, np.uint64), _put(nw + 3, ro, np.uint64)
        elif k == "host_encode":
            inputs["host"] = s[:p["n"]].copy() if err is None else inputs.pop("bad")[:p["n"]]
            host_result["words"] = oracle.encode(s[:p["n"]])
        else:  # the k-mer scans
            n, kk = p["n"], p["k"]
            if kd.reads == "packed":
                base = oracle.decode(w[:(n + 31) // 32], n)
                if k == "host_multi_packed":
                    inputs["host"] = w[:(n + 31) // 32].copy()
            else:
                base = s[AT7:AT7 + n] if k == "count_at7" else s[:n]
                if k == "host_hits":
                    inputs["host"] = base.copy() if err is None else inputs.pop("bad")[:n]
            if "queries" in p:
                inputs["queries"], inputs["taus"] = np.array(p["queries"], np.uint64), np.array(p["taus"], np.uint32)
                counts = np.array([int((oracle.kmer_hdist_scan(base, kk, _mask(q, kk)) <= t).sum()) for q, t in zip(p["queries"], p["taus"])], np.uint64)
                if kd.host:
                    host_result["counts"] = counts
                else:
                    outs["counts"] = _put(p["nq"] + 2, counts, np.uint64)
            else:
                dist = oracle.kmer_hdist_scan(base, kk, _mask(p["query"], kk))
                hit = np.flatnonzero(dist <= p["tau"])
                if k in ("scan", "scan_packed"):
                    outs["dist"] = _put(len(dist) + GUARD, dist, np.uint8)
                elif k == "host_hits":
                    host_result["pos"], host_result["dist"] = hit.astype(np.uint64), dist[hit]
                else:
                    cell = len(hit)
                    if k in ("hits", "hits_packed"):
                        m = min(p["cap"], len(hit))
                        outs["pos"] = _put(p["cap"] + 2, hit[:m].astype(np.uint64), np.uint64)
                        outs["hit_dist"] = _put(p["cap"] + GUARD, dist[hit[:m]], np.uint8)
        steps.append(Step(op, src, inputs, outs, cell, err is not None, raises, host_result))
    reports = []
    found = pending[0] if pending else None
    if deferred:
        if found:
            deferred.append(found)
        reports = deferred
    elif found:
        reports = [found]
    return steps, buf, reports


# ---- the growth queue (test_scratch_grows_in_the_middle_of_a_queue) ---------------------------------------------------------------------
def growth_plan():
    """One queue on a fresh context: a result pending, then each shared slot reallocated behind it.  (step, argument, slot -> bytes asked for).
    Every request of a slot must exceed 1.5 x the capacity before it + 4 KiB, so that the slot reallocates whatever the growth rule's head-room was
    (tests/test_queue_plan.py asserts that margin from the formulas): sizes found by walking the rule, not by hand."""
    L = READS[0]
    wpr = (L + 31) // 32

    def reads_for(slot7_bytes, slot6_bytes):
        """the smallest count of 150-base reads whose table-driven batch asks for more than both"""
        count = 1
        while True:
            b6, b7 = batch_scratch_bytes(count * wpr)
            if b6 > slot6_bytes and b7 > slot7_bytes:
                return count
            count += max(1, count // 64)

    def bases_for(nbytes):
        """the smallest hit-list input (16-byte aligned) whose scratch is more than nbytes"""
        rounds = 1
        while hits_scratch_bytes((rounds + HITS_ROUNDS - 1) // HITS_ROUNDS + 2) <= nbytes:
            rounds += max(1, rounds // 64)
        return 1024 * rounds + 32 + 5

    cap = {SLOT_PAD_PLAN: 0, SLOT_TILES: 0, SLOT_MULTI: 0}
    steps = []

    def add(kind, arg, asks):
        for slot, b in asks.items():
            cap[slot] = scratch_capacity(cap[slot], b)
        steps.append((kind, arg, asks))

    def margin(slot):
        return cap[slot] + cap[slot] // 2 + 4096

    n0 = 300_005
    add("hits", n0, {SLOT_TILES: hits_scratch_bytes(hits_trips(n0))})
    add("multi", 1, {SLOT_MULTI: multi_scratch_bytes(1)})
    for _ in range(2):
        count = reads_for(margin(SLOT_TILES), margin(SLOT_PAD_PLAN))
        b6, b7 = batch_scratch_bytes(count * wpr)
        add("batch", count, {SLOT_PAD_PLAN: b6, SLOT_TILES: b7})
        if len(steps) == 3:
            add("host_hits", 70_001, {})
            add("multi", 17, {SLOT_MULTI: multi_scratch_bytes(17)})
    for _ in range(2):
        n = bases_for(margin(SLOT_TILES))
        add("hits", n, {SLOT_TILES: hits_scratch_bytes(hits_trips(n))})
        if len(steps) == 7:
            add("host_multi", 17, {})
    add("multi", 40, {SLOT_MULTI: multi_scratch_bytes(40)})
    return steps


def expect_hits(oracle, s, k, query, tau, cap):
    """(n_hits, pos buffer of cap + 2, hit_dist buffer of cap + GUARD) of a hit list on the bases s, guards 0xA5"""
    dist = oracle.kmer_hdist_scan_threaded(s, k, _mask(query, k))
    hit = np.flatnonzero(dist <= tau)
    m = min(cap, len(hit))
    return len(hit), _put(cap + 2, hit[:m].astype(np.uint64), np.uint64), _put(cap + GUARD, dist[hit[:m]], np.uint8)


def expect_multi(oracle, s, k, queries, taus):
    return np.array([int((oracle.kmer_hdist_scan_threaded(s, k, _mask(int(q), k)) <= t).sum()) for q, t in zip(queries, taus)], np.uint64)


def expect_reads(oracle, s, L, count):
    """the words of `count` back-to-back reads of L bases, one encode() per read as the reference's idiom has it, + 2 guard words"""
    return _put(count * ((L + 31) // 32) + 2, np.concatenate([oracle.encode(s[r * L:(r + 1) * L]) for r in range(count)]), np.uint64)


def graph_queue():
    """one operation of every asynchronous kind, sizes with several count workgroups, the ASCII readers of `seq` first (an invalid byte planted in
    `seq` for the last replays is then the first captured launch's to report), nucgen after them"""
    first = [k.name for k in KINDS if not k.host and k.reads == "ascii"]
    rest = [k.name for k in KINDS if not k.host and k.reads != "ascii"]
    ops = []
    for t, kind in enumerate(first + rest):
        r = 0
        while True:  # the first occurrence with bytes to examine and a size of several workgroups
            p = params(kind, r)
            if p.get("n", 70_001) >= 70_001 and p.get("count", 256) >= 256 and p.get("slen", 70_001) >= 70_001:
                break
            r += 1
        ops.append(Op(t, kind, p))
    return Queue(-1, ops, {})


def graph_rounds(queue):
    """The ordinary calls issued after each of three replays: reads of a table-driven batch, bases of a hit list, queries of a multi-query count, each
    asking for more than the slot holds at that point (walked with ensure_scratch's rule from the recorded queue's own requests)."""
    lay = layouts()
    cap = {SLOT_PAD_PLAN: 0, SLOT_TILES: 0, SLOT_MULTI: 0}
    for op in queue.ops:  # the warm-up run before the capture
        asks = {}
        if op.kind in ("encode_tables", "decode_tables"):
            asks[SLOT_PAD_PLAN], asks[SLOT_TILES] = batch_scratch_bytes(int(lay[op.p["layout"]][1][-1]))
        elif op.kind in ("hits", "hits_cap0", "hits_packed"):
            asks[SLOT_TILES] = hits_scratch_bytes(hits_trips(op.p["n"]))
        elif op.kind in ("multi", "multi_packed"):
            asks[SLOT_MULTI] = multi_scratch_bytes(op.p["nq"])
        for slot, b in asks.items():
            cap[slot] = scratch_capacity(cap[slot], b)
    wpr = (READS[0] + 31) // 32
    out = []
    for _ in range(3):
        reads = 1
        while batch_scratch_bytes(reads * wpr)[1] <= cap[SLOT_TILES] or batch_scratch_bytes(reads * wpr)[0] <= cap[SLOT_PAD_PLAN]:
            reads += max(1, reads // 64)
        b6, b7 = batch_scratch_bytes(reads * wpr)
        cap[SLOT_PAD_PLAN], cap[SLOT_TILES] = scratch_capacity(cap[SLOT_PAD_PLAN], b6), scratch_capacity(cap[SLOT_TILES], b7)
        rounds = 1
        while hits_scratch_bytes((rounds + HITS_ROUNDS - 1) // HITS_ROUNDS + 2) <= cap[SLOT_TILES]:
            rounds += max(1, rounds // 64)
        n = 1024 * rounds + 32 + 5
        cap[SLOT_TILES] = scratch_capacity(cap[SLOT_TILES], hits_scratch_bytes(hits_trips(n)))
        nq = cap[SLOT_MULTI] // TABLE_BYTES + 1
        cap[SLOT_MULTI] = scratch_capacity(cap[SLOT_MULTI], multi_scratch_bytes(nq))
        out.append({"reads": reads, "hits_n": n, "nq": nq})
    return out
