"""GPU tests of QUEUES of mixed asynchronous calls with one sync at the end (tests/queue_plan.py is the plan and the host model): every ordered pair of
operation kinds adjacent once on a fresh context, context scratch growing in the middle of a queue, one hipGraph holding every family while ordinary calls
share its scratch slots, and two contexts running queues at the same time.  What is under test is what a context carries from one launch to the next:
the accumulators and tickets of the single-launch reductions, the scratch slots the families share, the ring of error slots and its FIFO of deferred errors."""
import functools
import threading

import numpy as np
import pytest

import queue_plan as qp

pytestmark = pytest.mark.gpu
FILL64_I = qp.FILL64 - 2**64  # the fill as torch's signed 64-bit type holds it


def _t(a):
    """numpy -> device tensor (the unsigned 64- and 32-bit types as their signed views)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _h(t, dtype):
    return t.cpu().numpy().view(dtype)


def _fresh_context():
    import bitnuc_amd as bn
    from bitnuc_amd import build
    build.ensure_built()
    c = bn.Context(0)
    c.set_variant("force_gpu", 1)
    return c


@functools.lru_cache(maxsize=None)
def _model(index, salt=0):
    """(steps, final shared buffers, sync reports) of plan queue `index`: computed once, shared by the tests, never changed"""
    import oracle_py
    return qp.model(qp.plan()[index], oracle_py, salt=salt)


def _size(op):
    return {key: v for key, v in op.p.items() if key in ("n", "k", "tau", "count", "stride", "L", "layout", "nq", "cap", "slen", "idx", "len")}


class Device:
    """everything a queue needs in device memory, allocated and uploaded before its first call"""

    def __init__(self, c, steps, init):
        import bitnuc_amd as bn
        self.shared = {name: _t(a) for name, a in init.items()}
        self.cells = _t(np.full(len(steps) + 2, qp.FILL64, np.uint64))
        self.lay, self.plans = {}, {}
        for name, (off, wo) in qp.layouts().items():
            d_off, d_wo = _t(off), _t(wo)
            self.lay[name] = (d_off, d_wo, len(off) - 1, int(wo[-1]))
            self.plans[name] = bn.BatchPlan(c, d_off, len(off) - 1)  # synchronous: before the queue
            assert self.plans[name].total_words == int(wo[-1])
        self.inp = [{name: _t(a) for name, a in st.inputs.items() if name != "host"} for st in steps]
        self.out = [{name: _t(np.full(a.size, qp.FILL if a.dtype == np.uint8 else qp.FILL64, a.dtype)) for name, a in st.outs.items()} for st in steps]

    def refill(self, init):
        """new data in place (the tensors a graph recorded keep their addresses)"""
        for name, a in init.items():
            self.shared[name].copy_(_t(a))
        self.cells.fill_(FILL64_I)
        for outs in self.out:
            for t in outs.values():
                t.fill_(qp.FILL if t.dtype.itemsize == 1 else FILL64_I)

    def close(self):
        for p in self.plans.values():
            p.close()


def _issue(c, st, x, D):
    """enqueue operation x of the queue; a host kind returns {name: result} or the (byte, index) it raised"""
    import bitnuc_amd as bn
    k, p = st.op.kind, st.op.p
    S, out, cell = D.shared, D.out[x], D.cells[x + 1:]
    src = D.inp[x].get("bad", S[st.src] if st.src else None)
    words = S["words"]
    if qp.KIND[k].host:
        try:
            if k == "host_encode":
                return {"words": c.encode_array(st.inputs["host"])}
            if k == "host_hits":
                pos, dist = c.kmer_hdist_hits(st.inputs["host"], p["k"], p["query"], p["tau"], with_dist=True)
                return {"pos": pos, "dist": dist}
            return {"counts": c.kmer_hdist_count_multi_packed(st.inputs["host"], p["n"], p["k"], st.inputs["queries"], st.inputs["taus"])}
        except bn.NucleotideError as e:
            return (e.byte, e.index) if e.kind == "InvalidBase" else (e.kind,)
    if k == "nucgen":
        c.nucgen_dev(S["seq"], p["n"], p["seed"], 0, p["flags"])
    elif k == "encode":
        c.encode_dev(src, p["n"], out.get("words", words))
    elif k == "decode":
        c.decode_dev(words, (p["n"] + 31) // 32, p["n"], S["seq2"])
    elif k in ("encode_tables", "decode_tables", "encode_plan", "decode_plan"):
        d_off, d_wo, count, total = D.lay[p["layout"]]
        if k == "encode_tables":
            c.encode_batch_dev(src, d_off, d_wo, count, total, out["words"])
        elif k == "decode_tables":
            c.decode_batch_dev(words, d_wo, d_off, count, total, out["back"])
        elif k == "encode_plan":
            D.plans[p["layout"]].encode_dev(src, out["words"])
        else:
            D.plans[p["layout"]].decode_dev(words, out["back"])
    elif k == "encode_fixed":
        c.encode_fixed_dev(src, p["L"], p["stride"], p["count"], out["words"])
    elif k == "decode_fixed_gap":
        c.decode_fixed_dev(words, p["L"], p["stride"], p["count"], out["back"])
    elif k in ("kmers_dense", "kmers_windows"):
        c.as_2bit_batch_dev(src, p["k"], p["stride"], p["count"], out["kmers"])
    elif k == "scan":
        c.kmer_hdist_scan_dev(src, p["n"], p["k"], p["query"], out["dist"])
    elif k == "count_aligned":
        c.kmer_hdist_count_dev(src, p["n"], p["k"], p["query"], p["tau"], cell)
    elif k == "count_at7":
        c.kmer_hdist_count_dev(src[qp.AT7:], p["n"], p["k"], p["query"], p["tau"], cell)
    elif k == "scan_packed":
        c.kmer_hdist_scan_packed_dev(words, (p["n"] + 31) // 32, p["n"], p["k"], p["query"], out["dist"])
    elif k == "count_packed":
        c.kmer_hdist_count_packed_dev(words, (p["n"] + 31) // 32, p["n"], p["k"], p["query"], p["tau"], cell)
    elif k == "hits":
        c.kmer_hdist_hits_dev(src, p["n"], p["k"], p["query"], p["tau"], out["pos"], out["hit_dist"], p["cap"], cell)
    elif k == "hits_cap0":
        c.kmer_hdist_hits_dev(src, p["n"], p["k"], p["query"], p["tau"], None, None, 0, cell)
    elif k == "hits_packed":
        c.kmer_hdist_hits_packed_dev(words, (p["n"] + 31) // 32, p["n"], p["k"], p["query"], p["tau"], out["pos"], out["hit_dist"], p["cap"], cell)
    elif k == "multi":
        c.kmer_hdist_count_multi_dev(src, p["n"], p["k"], D.inp[x]["queries"], D.inp[x]["taus"], p["nq"], out["counts"])
    elif k == "multi_packed":
        c.kmer_hdist_count_multi_packed_dev(words, (p["n"] + 31) // 32, p["n"], p["k"], D.inp[x]["queries"], D.inp[x]["taus"], p["nq"], out["counts"])
    elif k == "hdist":
        nw = (p["n"] + 31) // 32
        c.hdist_dev(words, nw, S["words_b"], nw, p["n"], cell)
    elif k == "base_counts":
        c.base_counts_dev(words, (p["n"] + 31) // 32, p["n"], out["counts"])
    elif k == "hdist_pairs":
        c.hdist_pairs_dev(words, S["words_b"], p["count"], p["len"], out["dist"])
    elif k == "hdist_query":
        c.hdist_query_dev(p["query"], words, p["count"], p["len"], out["dist"])
    elif k == "split":
        c.split_packed_dev(words, (p["slen"] + 31) // 32, p["slen"], p["idx"], out["left"], out["right"])
    else:
        raise KeyError(k)
    return None


def _first_difference(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else f"{d.size} of {want.size} differ, first at {int(d[0])}: got {got[d[0]]!r}, expected {want[d[0]]!r}"


def _compare(qindex, steps, final, D, host_results):
    """every output of the queue against the model -> [(queue, position, kind, size, previous kind, what)]"""
    bad = []
    cells = _h(D.cells, np.uint64)

    def report(x, what):
        st = steps[x]
        bad.append((qindex, x, st.op.kind, _size(st.op), steps[x - 1].op.kind if x else None, what))

    for x, st in enumerate(steps):
        want_cell = qp.FILL64 if st.cell is None else st.cell
        if not (st.unspecified and st.cell is not None) and int(cells[x + 1]) != want_cell:
            report(x, f"cell: got {int(cells[x + 1]):#x}, expected {want_cell:#x}")
        if st.op.kind in qp.HOST_KINDS:
            got = host_results[x]
            if st.raises is not None:
                if got != tuple(st.raises):
                    report(x, f"host call: got {got!r}, expected InvalidBase {st.raises!r}")
                continue
            if not isinstance(got, dict):
                report(x, f"host call raised {got!r}")
                continue
            for name, want in st.host_result.items():
                d = _first_difference(np.asarray(got[name]), want)
                if d:
                    report(x, f"host {name}: {d}")
            continue
        if st.unspecified:
            continue
        for name, want in st.outs.items():
            d = _first_difference(_h(D.out[x][name], want.dtype), want)
            if d:
                report(x, f"{name}: {d}")
    if int(cells[0]) != qp.FILL64 or int(cells[-1]) != qp.FILL64:
        bad.append((qindex, None, "cells", None, None, "a guard cell was written"))
    for name in ("seq", "seq2", "words", "words_b"):
        d = _first_difference(_h(D.shared[name], final[name].dtype), final[name])
        if d:
            bad.append((qindex, None, name, None, None, f"final state: {d}"))
    return bad


def _syncs(c, reports):
    """the syncs after a queue: one report each in the model's order, then a clean one -> list of mismatches"""
    import bitnuc_amd as bn
    bad = []
    for n, want in enumerate(list(reports) + [None]):
        try:
            c.sync()
            got = None
        except bn.NucleotideError as e:
            got = (e.byte, e.index) if e.kind == "InvalidBase" else (e.kind,)
        if got != (tuple(want) if want else None):
            bad.append(f"sync {n + 1}: got {got!r}, expected {want!r}")
    return bad


def _run_queue(c, qindex, steps, final, reports, init):
    """the whole queue on context c with nothing but the stream between its calls -> failures"""
    import torch
    D = Device(c, steps, init)
    torch.cuda.synchronize()
    host_results = {}
    for x, st in enumerate(steps):
        r = _issue(c, st, x, D)
        if st.op.kind in qp.HOST_KINDS:
            host_results[x] = r
    bad = [(qindex, None, "sync", None, None, m) for m in _syncs(c, reports)]
    bad += _compare(qindex, steps, final, D, host_results)
    D.close()
    return bad


@pytest.mark.parametrize("index", range(len(qp.plan())), ids=lambda i: f"q{i}" + ("-errors" if qp.plan()[i].errors else ""))
def test_every_adjacent_pair_in_one_queue(oracle, index):
    """One plan queue on a fresh context: everything allocated and uploaded first, every call issued with no sync, copy or read-back in between, then the
    syncs.  A clean queue's sync returns OK.  In an error queue two ASCII operations i < j read a private copy of their input with one invalid byte: the
    first sync raises InvalidBase with i's byte and index (relative to that call's input), and the syncs after it are clean -- except where the header's
    FIFO rule applies: a host-pointer call between i and j has drained and deferred i, so j is found by the sync's own drain, queued behind i and reported
    by the second sync; the third is clean.  A host kind returns its own result synchronously and correctly and swallows nothing: with i before it, it
    returns OK and the next sync still reports i; when it is j, it raises its own InvalidBase at once and the next sync reports i.  Then every output --
    private buffers with their 0xA5 guards, the packed result cells, the final state of the shared buffers -- is compared with the model, failures listed
    as (queue, position, kind, size, previous kind, what)."""
    steps, final, reports = _model(index)
    c = _fresh_context()
    try:
        bad = _run_queue(c, index, steps, final, reports, qp.initial_buffers(oracle))
    finally:
        c.close()
    assert not bad, "\n".join(map(repr, bad[:20])) + f"\n({len(bad)} failures)"


def _reads_batch(oracle, count, seed):
    """`count` back-to-back reads: device sequence, offsets, word offsets, 0xA5 output and the oracle's words"""
    L = qp.READS[0]
    wpr = (L + 31) // 32
    s = oracle.nucgen(count * L, seed)
    off, wo = np.arange(count + 1, dtype=np.int64) * L, np.arange(count + 1, dtype=np.int64) * wpr
    want = qp.expect_reads(oracle, s, L, count)
    return {"seq": _t(s), "off": _t(off), "wo": _t(wo), "count": count, "total": count * wpr, "out": _t(np.full(want.size, qp.FILL64, np.uint64)), "want": want}


def _issue_reads(c, b):
    c.encode_batch_dev(b["seq"], b["off"], b["wo"], b["count"], b["total"], b["out"])


def _hits_call(oracle, n, seed, k=21, tau=15, cap=4099):
    s = oracle.nucgen(n, seed, 0, 2)
    query = qp._mix(seed)
    n_hits, pos, hd = qp.expect_hits(oracle, s, k, query, tau, cap)
    return {"seq": _t(s), "n": n, "k": k, "query": query, "tau": tau, "cap": cap, "pos": _t(np.full(pos.size, qp.FILL64, np.uint64)),
            "hd": _t(np.full(hd.size, qp.FILL, np.uint8)), "cell": _t(np.full(3, qp.FILL64, np.uint64)), "want": (n_hits, pos, hd)}


def _issue_hits(c, b):
    c.kmer_hdist_hits_dev(b["seq"], b["n"], b["k"], b["query"], b["tau"], b["pos"], b["hd"], b["cap"], b["cell"][1:])


def _check_hits(b, what, bad):
    n_hits, pos, hd = b["want"]
    cell = _h(b["cell"], np.uint64)
    if [int(v) for v in cell] != [qp.FILL64, n_hits, qp.FILL64]:
        bad.append((what, f"n_hits cell and its guards: {[hex(int(v)) for v in cell]}, expected {n_hits}"))
    for name, t, want in (("pos", b["pos"], pos), ("hit_dist", b["hd"], hd)):
        d = _first_difference(_h(t, want.dtype), want)
        if d:
            bad.append((what, f"{name}: {d}"))


def _multi_call(oracle, s, d_seq, nq, seed, k=16):
    queries = np.array([qp._mix(seed + j) for j in range(nq)], np.uint64)
    taus = np.array([qp._taus(k)[j % 4] for j in range(nq)], np.uint32)
    return {"seq": d_seq, "n": s.size, "k": k, "nq": nq, "queries": _t(queries), "taus": _t(taus), "hq": queries, "ht": taus,
            "out": _t(np.full(nq + 2, qp.FILL64, np.uint64)), "want": qp._put(nq + 2, qp.expect_multi(oracle, s, k, queries, taus), np.uint64)}


def _issue_multi(c, b):
    c.kmer_hdist_count_multi_dev(b["seq"], b["n"], b["k"], b["queries"], b["taus"], b["nq"], b["out"])


def _check_words(b, what, bad, key="out"):
    d = _first_difference(_h(b[key], np.uint64), b["want"])
    if d:
        bad.append((what, d))


def test_scratch_grows_in_the_middle_of_a_queue(oracle):
    """One context, one queue, one sync: a hit list pending, then every shared scratch slot reallocated behind it (queue_plan.growth_plan: each request
    more than 1.5 x the capacity before it + 4 KiB) -- table-driven batches grow slots 6 and 7 under the pending hit list, two longer hit lists grow slot 7
    past one and past four tiles of per-trip counts, multi-query counts of 1, 17 and 40 queries grow slot 8, host hits and a host multi-query count use
    the staging slots in between.  Growth of a buffer no graph holds waits for the stream and frees it: what was queued before must have finished with it.
    Every output, the earliest included, is compared."""
    import torch
    plan = qp.growth_plan()
    small = oracle.nucgen(300_005, 77, 0, 2)
    d_small = _t(small)
    calls = []
    for t, (kind, arg, asks) in enumerate(plan):
        if kind == "hits":
            calls.append((kind, _hits_call(oracle, arg, 500 + t)))
        elif kind == "batch":
            calls.append((kind, _reads_batch(oracle, arg, 600 + t)))
        elif kind == "multi":
            calls.append((kind, _multi_call(oracle, small[:131_077], d_small, arg, 700 + t)))
        elif kind == "host_hits":
            h = small[:arg]
            calls.append((kind, {"h": h, "want": qp.expect_hits(oracle, h, 21, 12345, 15, h.size)}))
        else:
            h = small[:70_001]
            b = _multi_call(oracle, h, None, arg, 800 + t)
            calls.append((kind, b))
    c = _fresh_context()
    bad = []
    try:
        torch.cuda.synchronize()
        for kind, b in calls:
            if kind == "hits":
                _issue_hits(c, b)
            elif kind == "batch":
                _issue_reads(c, b)
            elif kind == "multi":
                _issue_multi(c, b)
            elif kind == "host_hits":
                pos, dist = c.kmer_hdist_hits(b["h"], 21, 12345, 15, with_dist=True)
                n_hits, wpos, wd = b["want"]
                if pos.size != n_hits or not np.array_equal(pos, wpos[:n_hits]) or not np.array_equal(dist, wd[:n_hits]):
                    bad.append((kind, "host hit list differs"))
            else:
                got = c.kmer_hdist_count_multi(small[:70_001], b["k"], b["hq"], b["ht"])
                if not np.array_equal(got, b["want"][:b["nq"]]):
                    bad.append((kind, "host counts differ"))
        c.sync()
        for t, (kind, b) in enumerate(calls):
            what = (t, kind, plan[t][1])
            if kind == "hits":
                _check_hits(b, what, bad)
            elif kind in ("batch", "multi"):
                _check_words(b, what, bad)
    finally:
        c.close()
    assert not bad, "\n".join(map(repr, bad[:20]))


def test_one_graph_holds_every_family_and_ordinary_calls_share_its_scratch(oracle):
    """After a warm-up run, ONE hipGraph records a queue with every asynchronous kind (queue_plan.graph_queue; linear on the context's stream): the captured
    slots are its ASCII-reading launches, one per call.  Three times: new data in place, replay, then ORDINARY calls of the families that share the
    recorded launches' scratch slots at sizes that outgrow them (a table-driven batch and a hit list: slots 6 and 7; a multi-query count with more
    queries: slot 8; sizes from queue_plan.graph_rounds), one sync, the replay's outputs against the model and the ordinary calls' against the oracle.
    The buffers the graph recorded are retired, not freed: churn allocations filled with 0x5A stay intact.  Then a replay on an invalid byte is
    reported once, with the first captured launch's byte and index, and the replay after it is clean."""
    import torch
    import bitnuc_amd as bn
    from bitnuc_amd import build
    build.ensure_built()
    queue = qp.graph_queue()
    rounds = qp.graph_rounds(queue)
    assert {o.kind for o in queue.ops} == {k.name for k in qp.KINDS if not k.host}
    models = [qp.model(queue, oracle, salt=salt) for salt in range(4)]
    s = torch.cuda.Stream()
    bad = []
    with torch.cuda.stream(s):
        c = bn.Context(0, stream=s.cuda_stream)
        c.set_variant("force_gpu", 1)
        steps = models[0][0]
        D = Device(c, steps, qp.initial_buffers(oracle, 0))
        big = oracle.nucgen(131_077, 91, 0, 2)
        d_big = _t(big)
        extra = [{"reads": _reads_batch(oracle, r["reads"], 40 + t), "hits": _hits_call(oracle, r["hits_n"], 50 + t), "multi": _multi_call(oracle, big, d_big, r["nq"], 60 + t)}
                 for t, r in enumerate(rounds)]
        torch.cuda.synchronize()
        for x, st in enumerate(steps):  # warm-up: scratch grows here, outside the capture
            _issue(c, st, x, D)
        c.sync()
        assert c.get("captured_slots") == 0
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                for x, st in enumerate(steps):
                    _issue(c, st, x, D)
            assert c.get("captured_slots") == sum(qp.takes_slot(o) for o in queue.ops)
            churn = []
            for t in range(3):
                steps, final, reports = models[t + 1]
                D.refill(qp.initial_buffers(oracle, t + 1))
                g.replay()
                e = extra[t]
                _issue_reads(c, e["reads"])   # slots 6 and 7: after the recorded hit lists and batches
                _issue_hits(c, e["hits"])     # slot 7 again
                _issue_multi(c, e["multi"])   # slot 8: more queries than the recorded multi-query counts
                bad += [(t, m) for m in _syncs(c, reports)]
                bad += _compare(f"replay {t}", steps, final, D, {})
                _check_words(e["reads"], (t, "ordinary batch"), bad)
                _check_hits(e["hits"], (t, "ordinary hits"), bad)
                _check_words(e["multi"], (t, "ordinary multi"), bad)
                churn += [torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda:0") for _ in range(16)]
            assert not bad, "\n".join(map(repr, bad[:20]))
            # a replay on an invalid byte: the first captured launch (the bulk encode of `seq`) reports it, once
            first = queue.ops[0]
            assert first.kind == "encode" and first.p["n"] > 33_333
            D.refill(qp.initial_buffers(oracle, 0))
            D.shared["seq"][33_333] = ord("N")
            g.replay()
            assert _syncs(c, [(ord("N"), 33_333)]) == []
            D.refill(qp.initial_buffers(oracle, 0))
            g.replay()
            assert _syncs(c, []) == []
            steps, final, reports = models[0]
            bad += _compare("last replay", steps, final, D, {})
            assert not bad, "\n".join(map(repr, bad[:20]))
            assert all(bool((t == 0x5A).all()) for t in churn), "a replay or an ordinary call wrote into memory that had been given back"
        finally:
            g.reset()
            del g
            D.close()
            c.close()


def test_two_contexts_run_queues_at_the_same_time(oracle):
    """Two threads, each with its own context on device 0 and its own plan queue (both hold k-mer counts, hit lists and multi-query counts), three runs each
    with a sync after each run: the accumulators, tickets, scratch and error slots are per context, so both compare with the model every time."""
    plan = qp.plan()
    want = {"count_aligned", "hits", "multi", "count_packed"}
    picks = [q.index for q in plan if not q.errors and want <= {o.kind for o in q.ops}][:2]
    if len(picks) < 2:
        picks = [q.index for q in plan if not q.errors and len(want & {o.kind for o in q.ops}) >= 3][:2]
    assert len(picks) == 2
    inits = qp.initial_buffers(oracle)
    models = {i: _model(i) for i in picks}  # computed in the main thread
    failures, errors = [], []

    def worker(index):
        try:
            c = _fresh_context()
            try:
                steps, final, reports = models[index]
                for run in range(3):
                    failures.extend((run,) + f for f in _run_queue(c, index, steps, final, reports, inits))
            finally:
                c.close()
        except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in picks]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    assert not failures, "\n".join(map(repr, failures[:20]))
