"""The plan of the asynchronous-queue tests (tests/queue_plan.py), checked without a GPU: the pair coverage of its order, its errors, its kind table
against the header, the constants and byte formulas its sizes rest on against the sources' text, and the arithmetic of the scratch-growth queues."""
import os
import re

import numpy as np

import alphabet
import queue_plan as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitnuc_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(fname, name):
    m = re.search(r"constexpr\s+(?:unsigned\s+)?(?:int|unsigned|size_t)\s+" + name + r"\s*=\s*(\d+)\s*;", _src(fname))
    assert m, (fname, name)
    return int(m.group(1))


def test_every_ordered_pair_is_adjacent_in_some_queue():
    n = len(qp.KINDS)
    circ = qp.euler_circuit(n)
    assert len(circ) == n * n + 1 and circ[0] == circ[-1] == 0
    assert len(set(zip(circ, circ[1:]))) == n * n  # every ordered pair, self-loops included, exactly once
    plan = qp.plan()
    pairs = set()
    for q in plan:
        kinds = [o.kind for o in q.ops]
        pairs |= set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in qp.NAMES for b in qp.NAMES}
    # cut with one operation of overlap: nothing lost, nothing twice
    assert sum(len(q.ops) - 1 for q in plan) == n * n
    for a, b in zip(plan, plan[1:]):
        assert a.ops[-1] == b.ops[0]


def test_queue_lengths_and_kind_spread():
    plan = qp.plan()
    assert all(2 <= len(q.ops) <= qp.MAX_QUEUE <= 64 for q in plan)
    for name in qp.NAMES:
        assert sum(any(o.kind == name for o in q.ops) for q in plan) >= 3, name


def test_sizes_reach_the_paths_the_issue_names():
    ops = [o for q in qp.plan() for o in q.ops]
    for kind in ("count_aligned", "count_at7", "count_packed", "hits", "hits_cap0", "hits_packed", "scan", "scan_packed", "multi", "multi_packed"):
        mine = [o.p for o in ops if o.kind == kind]
        assert any(p["n"] < p["k"] for p in mine), kind            # no windows: the memset path, no ticket
        assert any(p["n"] == p["k"] + 5 for p in mine), kind       # tail windows only
        wgs = {-(-(p["n"] - p["k"] + 1) // qp.COUNT_WG_WINDOWS) for p in mine if p["n"] > 1000}
        assert min(wgs) <= 5 and max(wgs) >= 18 and len(wgs) >= 3, (kind, wgs)
        assert {p["k"] for p in mine} == set(qp.KS)
        assert {0, 1} <= {p["tau"] for p in mine} and any(p["tau"] == p["k"] for p in mine) and any(p["tau"] == 3 * p["k"] // 4 for p in mine)
    for kind in ("multi", "multi_packed"):
        mine = [o.p for o in ops if o.kind == kind]
        assert {p["nq"] for p in mine} == {1, qp.MULTI_QB, qp.MULTI_QB + 1}
        for p in mine:  # one query repeated under different high bits
            if p["nq"] > 1 and p["k"] < 32:
                low = (1 << (2 * p["k"])) - 1
                assert p["queries"][0] & low == p["queries"][1] & low and p["queries"][0] != p["queries"][1]
    lay = qp.layouts()
    assert 1000 <= len(lay["reads"][0]) - 1 <= 4000 and 1000 <= len(lay["ragged"][0]) - 1 <= 4000
    lens = np.diff(lay["ragged"][0])
    assert (lens == 0).sum() > 100 and len(set(lens.tolist())) > 100 and set(np.diff(lay["reads"][0]).tolist()) == {150}
    assert any(o.p["stride"] == o.p["L"] + 3 for o in ops if o.kind == "decode_fixed_gap")
    assert {o.p["stride"] for o in ops if o.kind == "kmers_windows"} == {1}
    assert all(o.p["stride"] == o.p["k"] for o in ops if o.kind == "kmers_dense")


def test_errors_cover_every_ascii_kind_in_both_roles():
    plan = qp.plan()
    lay = qp.layouts()
    first, second, classes = set(), set(), set()
    nerr = 0
    for q in plan:
        if not q.errors:
            continue
        nerr += 1
        (i, (bi, pi)), (j, (bj, pj)) = sorted(q.errors.items())
        assert i < j
        for x, b, p in ((i, bi, pi), (j, bj, pj)):
            lo, hi = qp.examined(q.ops[x], lay)
            assert lo <= p < hi and b in alphabet.INVALID
            classes.add(alphabet.CLASS_OF[b])
        assert alphabet.CLASS_OF[bi] != alphabet.CLASS_OF[bj]
        first.add(q.ops[i].kind)
        second.add(q.ops[j].kind)
    assert first == second == set(qp.ASCII_KINDS) and classes == {"valid-selector", "other"}
    assert 0.3 <= nerr / len(plan) <= 0.4  # about a third of the queues


def test_kind_table_names_the_asynchronous_surface():
    """exactly the _dev symbols of the header that launch on the stream, plus the three host kinds; the exclusions are listed with their reasons"""
    header = open(os.path.join(ROOT, "include", "bitnuc_hip.h")).read()
    declared = set(re.findall(r"\b(bitnuc_[a-z0-9_]+)\s*\(", header))
    dev = {s for s in declared if s.endswith("_dev")}
    table = {k.symbol for k in qp.KINDS}
    assert {k.symbol for k in qp.KINDS if not k.host} == dev - set(qp.EXCLUDED_DEV_SYMBOLS)
    assert set(qp.EXCLUDED_DEV_SYMBOLS) <= dev and all(qp.EXCLUDED_DEV_SYMBOLS.values())
    assert {k.symbol for k in qp.KINDS if k.host} == {"bitnuc_encode", "bitnuc_kmer_hdist_hits", "bitnuc_kmer_hdist_count_multi_packed"} <= declared
    assert table <= declared
    # the host kinds go through the context: they drain what is pending and use the staging slots
    # (each names the host skeleton of ref_dispatch.h, which drains after the host-cutoff return and before the chunk loop)
    kmer = _src("kmer.hip")
    for sym in ("bitnuc_kmer_hdist_hits", "bitnuc_kmer_hdist_count_multi_packed"):
        body = kmer[kmer.index(f"int {sym}("):]
        assert "return ref_host(c, " in body[:body.index("\n}\n")], sym
    ref = _src("ref_dispatch.h")
    body = ref[ref.index("int ref_host("):]
    body = body[:body.index("\n}\n")]
    assert body.count("flush_pending(c, err)") == 1 and body.count("on_host(c, ") == 1 and body.count("host_loop(c, ") == 1
    assert body.index("on_host(c, ") < body.index("return bad >= 0 ?") < body.index("flush_pending(c, err)") < body.index("host_loop(c, ")
    codec = _src("codec.hip")
    body = codec[codec.index("int bitnuc_encode("):]
    assert "flush_pending(c, err)" in body[:body.index("\n}\n")]


def test_constants_and_formulas_are_the_sources():
    assert qp.K_BLOCK == _const("device_prims.h", "kBlock")
    assert qp.COUNT_ROUNDS == _const("runtime.h", "kCountRounds")
    assert qp.HITS_ROUNDS == _const("scan_hits_device.h", "kHitsRounds")
    assert qp.HITS_TILE == _const("scan_hits_device.h", "kHitsTile")
    assert qp.MULTI_QB == _const("scan_multi_device.h", "kMultiQB")
    assert qp.BATCH_TILE == _const("batch_device.h", "kBatchTile")
    kmer, batch, rt, rth = _src("kmer.hip"), _src("batch.hip"), _src("runtime.hip"), _src("runtime.h")
    # the scratch slots and the byte formulas, as they are written
    assert "const unsigned long long ntiles = (ntr + kHitsTile - 1) / kHitsTile, cbytes = (4 * ntr + 255) & ~255ull;" in kmer
    assert f"ensure_scratch(c, {qp.SLOT_TILES}, cbytes + 8 * ntiles, err)" in kmer
    assert "const unsigned long long ntr = hits_trips(n, skip) + 2;" in kmer
    assert "{ return (scan_rounds(n, skip) + kHitsRounds - 1) / kHitsRounds; }" in _src("scan_hits_device.h")
    assert f"ensure_scratch(c, {qp.SLOT_MULTI}, a.nq * sizeof(Count3MfmaTable), err)" in kmer
    assert "struct Count3MfmaTable { uint32_t w[64][12]; float c[4]; };" in _src("scan_mfma_host.h") and qp.TABLE_BYTES == 64 * 12 * 4 + 4 * 4
    assert "const size_t ntiles = (total_words + kBatchTile - 1) / kBatchTile;" in batch
    assert f"ensure_scratch(c, {qp.SLOT_PAD_PLAN}, total_words + 2 + kBatchTile, err)" in batch
    assert f"ensure_scratch(c, {qp.SLOT_TILES}, (ntiles + 1 + 2) * sizeof(unsigned long long), err)" in batch
    # the host loops' staging slots
    assert "ensure_scratch(c, 1, pcap * 8, err)" in kmer and "ensure_scratch(c, 3, 64, err)" in kmer and "ensure_scratch(c, 2, nq * 12, err)" in kmer
    # ensure_scratch's growth rule: max(bytes, 1.5 x old), 4 KiB granules; a buffer no graph holds is freed after a wait for the stream
    assert "size_t want = old_cap + old_cap / 2;" in rt and "if (want < bytes) want = bytes;" in rt and "size_t cap = (want + 4095) & ~(size_t)4095;" in rt
    assert re.search(r"c->retired_scratch\.push_back\(c->scratch\[which\]\);.*?\} else \{\s*HIPCHK\(hipStreamSynchronize\(c->stream\)\);\s*HIPCHK\(hipFree\(c->scratch\[which\]\)\);", rt, re.S)
    for old, b in ((0, 1), (0, 4096), (4096, 4097), (4096, 10_000), (8192, 8193), (12_288, 12_000)):
        want = old if b <= old else -(-max(b, old + old // 2) // 4096) * 4096
        assert qp.scratch_capacity(old, b) == want
    # the accumulators and tickets the plan's comments name
    assert "c->d_acc + 5, c->d_tickets + 2" in kmer and kmer.count("c->d_acc + 5, c->d_tickets + 2") >= 2  # the aligned count and the bit-plane count share them
    assert "c->d_acc + 6, c->d_tickets + 3" in kmer and "c->d_acc + 4), c->d_tickets + 1" in kmer
    assert "zero between launches" in rth
    assert qp.scan_rounds(1055) == 0 and qp.scan_rounds(1056) == 1 and "return nr >= 1056 ? (nr - 32) >> 10 : 0;" in _src("scan_mfma_host.h")
    assert qp.hits_scratch_bytes(75) == 512 + 8 and qp.hits_scratch_bytes(4097) == 16_640 + 16
    assert qp.batch_scratch_bytes(7500) == (7566, (118 + 3) * 8)


def test_growth_queue_reallocates_every_shared_slot_behind_a_pending_result():
    steps = qp.growth_plan()
    assert steps[0][0] == "hits"  # the pending result
    cap = {qp.SLOT_PAD_PLAN: 0, qp.SLOT_TILES: 0, qp.SLOT_MULTI: 0}
    grown = {s: 0 for s in cap}
    for kind, arg, asks in steps:
        for slot, b in asks.items():
            if cap[slot]:  # every later request: more than the growth rule's own head-room over what the slot holds, so it reallocates
                assert b > cap[slot] + cap[slot] // 2 + 4096, (kind, arg, slot, b, cap[slot])
                grown[slot] += 1
            cap[slot] = qp.scratch_capacity(cap[slot], b)
        if kind == "hits":
            assert asks[qp.SLOT_TILES] == qp.hits_scratch_bytes(qp.hits_trips(arg))
        if kind == "batch":
            assert (asks[qp.SLOT_PAD_PLAN], asks[qp.SLOT_TILES]) == qp.batch_scratch_bytes(arg * 5)
        if kind == "multi":
            assert asks[qp.SLOT_MULTI] == arg * qp.TABLE_BYTES
    assert grown == {qp.SLOT_PAD_PLAN: 1, qp.SLOT_TILES: 4, qp.SLOT_MULTI: 2}
    kinds = [s[0] for s in steps]
    assert kinds.count("batch") == 2 and kinds.count("hits") == 3 and [s[1] for s in steps if s[0] == "multi"] == [1, 17, 40]
    assert "host_hits" in kinds and "host_multi" in kinds
    trips = [qp.hits_trips(s[1]) for s in steps if s[0] == "hits"]
    assert trips[0] < 1024 < trips[1] and 2048 < trips[2] and trips[2] > 4 * qp.HITS_TILE  # more than one, then more than four tiles of per-trip counts
    # slot 7 is asked for by both families in turn: hit list, batch, batch, hit list, hit list
    assert [s[0] for s in steps if qp.SLOT_TILES in s[2]] == ["hits", "batch", "batch", "hits", "hits"]


def test_graph_queue_and_the_calls_that_outgrow_its_scratch():
    q = qp.graph_queue()
    assert sorted(o.kind for o in q.ops) == sorted(k.name for k in qp.KINDS if not k.host)
    first_nucgen = [o.kind for o in q.ops].index("nucgen")
    assert all(qp.KIND[o.kind].reads == "ascii" for o in q.ops[:first_nucgen]) and q.ops[0].kind == "encode"
    assert sum(qp.takes_slot(o) for o in q.ops) == sum(1 for k in qp.KINDS if k.reads == "ascii" and not k.host)
    lay = qp.layouts()
    cap7 = max([qp.scratch_capacity(0, qp.hits_scratch_bytes(qp.hits_trips(o.p["n"]))) for o in q.ops if o.kind.startswith("hits")] +
               [qp.scratch_capacity(0, qp.batch_scratch_bytes(int(lay[o.p["layout"]][1][-1]))[1]) for o in q.ops if o.kind.endswith("_tables")])
    cap8 = qp.scratch_capacity(0, max(o.p["nq"] for o in q.ops if o.kind.startswith("multi")) * qp.TABLE_BYTES)
    for r in qp.graph_rounds(q):
        b7 = qp.batch_scratch_bytes(r["reads"] * 5)[1]
        assert b7 > cap7
        cap7 = qp.scratch_capacity(cap7, b7)
        h7 = qp.hits_scratch_bytes(qp.hits_trips(r["hits_n"]))
        assert h7 > cap7
        cap7 = qp.scratch_capacity(cap7, h7)
        assert r["nq"] * qp.TABLE_BYTES > cap8
        cap8 = qp.scratch_capacity(cap8, r["nq"] * qp.TABLE_BYTES)


def test_model_reports_errors_as_the_header_orders_them(oracle):
    """the model's sync reports on the plan's error queues: the earlier operation first; the later one only where a host-pointer call drained in between
    (the FIFO of include/bitnuc_hip.h) or where the earlier one was a host call's own"""
    header = open(os.path.join(ROOT, "include", "bitnuc_hip.h")).read()
    assert "three syncs report A, B, C" in header and "kept in launch order, oldest first, one per bitnuc_ctx_sync" in header
    seen_two = seen_one = 0
    for q in qp.plan():
        if not q.errors:
            continue
        steps, final, reports = qp.model(q, oracle)
        (i, ei), (j, ej) = sorted(q.errors.items())
        host = [x for x, o in enumerate(q.ops) if qp.KIND[o.kind].host]
        i_host, j_host = i in host, j in host
        drained_between = any(i < h <= j for h in host)
        want = []
        if not i_host:
            want.append(ei)
        if not j_host and (i_host or drained_between):
            want.append(ej)
        assert [tuple(r) for r in reports] == [tuple(w) for w in want], q.index
        assert steps[i].unspecified and steps[j].unspecified and sum(s.unspecified for s in steps) == 2
        assert (steps[i].raises == ei) == i_host and (steps[j].raises == ej) == j_host
        seen_two += len(reports) == 2
        seen_one += len(reports) == 1
    assert seen_one >= 3 and seen_two >= 3
