"""CPU tests of bench.py's process model (no GPU touched: --rehearse-cpu).

`python bench.py --gpus N` with no launcher must start N fresh rank processes itself, relay
rank 0's single JSON line and return the ranks' worst exit code; a collective that stalls must be
visible in the line ("stalled": true) AND in the exit code -- never rc 0."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(*flags, timeout=240, **env_extra):
    env = dict(os.environ, **env_extra)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, BENCH, *flags], capture_output=True, text=True, timeout=timeout, env=env)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    return r.returncode, lines, r.stderr


def test_self_launch_two_ranks_prints_one_line():
    rc, lines, err = run("--gpus", "2", "--rehearse-cpu", "--backend", "gloo", "--steps", "5", "--warmup", "1", "--full")
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["warmup"] == 1
    assert line["value"] is None and "rehearsal" in line  # a rehearsal can never be mistaken for a measurement
    assert line["config"]["control_backend"] == "gloo" and line["rccl_ok"] is None
    # the N>1 line carries config 4's side measurements
    assert line["allgather_packed"]["own_slot_ok"] is True
    assert line["allgather_packed"]["all_slots_ok"] is True  # EVERY rank's slot of the gathered buffer against what it must hold
    assert "encode_allgather_end_to_end" in line
    assert "stalled" not in line and "collective_error" not in line
    # north_star's own split: a ragged batch by whole sequences, gather of unequal word counts (here: the exchange alone, slots hold their word indices)
    rb = line["ragged_batch_sharded"]
    assert rb["all_slots_ok"] is True and sum(rb["words_per_rank"]) == rb["total_words"] and len(set(rb["words_per_rank"])) == 2


def test_a_wrong_word_in_a_peer_slot_fails_the_run():
    """Config 4's check is literal: the gathered buffer is compared slot by slot with what every rank's shard must pack to (here, without a
    GPU, arange + rank), so a gather that delivered garbage into a PEER's slot is caught -- the line says so and the run exits 3."""
    rc, lines, err = run("--gpus", "2", "--rehearse-cpu", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--full", BITNUC_BENCH_PLANT_BAD_SLOT="1")
    # the rank exits 3 (as for parity_vs_oracle); the launcher folds a failed rank into its own non-zero code and names the FIRST failure it saw as the root
    # cause -- usually rank 0's "exitcode: 3", now and then its peer's, torn down while rank 0 was exiting (seen once in round 5): the line below is the evidence
    assert rc != 0, (rc, err[-2000:])
    line = json.loads(lines[0])
    assert line["allgather_packed"]["own_slot_ok"] is True and line["allgather_packed"]["all_slots_ok"] is False
    assert line["allgather_packed"]["first_bad_slot"] == 1  # rank 0 prints the line: the wrong word sits in its peer's slot


def test_stalled_collective_is_reported_and_fails():
    rc, lines, err = run("--gpus", "2", "--rehearse-cpu", "--backend", "gloo", "--steps", "3", "--warmup", "1",
                         "--inject-stall", "1", "--dist-timeout", "30", "--full")
    assert rc != 0, "a stalled collective must not exit 0"
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["stalled"] is True and "allgather" in line["stalled_stage"]


def test_plain_run_leaves_the_side_blocks_to_full():
    """Without --full a run times the step alone: no config-4 gathers (nor a stall in them), no CPU baseline; the line says so."""
    rc, lines, err = run("--gpus", "2", "--rehearse-cpu", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--inject-stall", "1", "--dist-timeout", "30")
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["config"]["full"] is False and line["steps"] == 3
    assert not {"allgather_packed", "encode_allgather_end_to_end", "ragged_batch_sharded", "c_abi_allgather", "cpu_baseline", "stalled"} & line.keys()


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--rehearse-cpu"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_steps_and_dump_outputs_arguments_are_checked():
    """--steps is the number of timed steps (at least one: ms_per_step is the timed time over it); --dump-outputs needs a step that computes."""
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--rehearse-cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
    r = subprocess.run([sys.executable, BENCH, "--rehearse-cpu", "--dump-outputs", "never_written"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and not os.path.exists("never_written")


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_results(tmp_path, oracle):
    """--dump-outputs DIR writes what the last timed step computed: the words its encode wrote (set (K - 1) % 3, seed SEED + 2 for K = 3) and
    the bases its decode wrote (set 0, seed SEED): every word of 93,751 (the tail word included) and a seeded sample of the 3,000,007 bases,
    each against the oracle; a second run with the same arguments writes the same files."""
    import numpy as np
    n, seed = 3_000_007, 0xB17C0DE
    runs = []
    for d in ("a", "b"):
        rc, lines, err = run("--gpus", "1", "--steps", "3", "--warmup", "1", "--bases", str(n), "--no-extras", "--no-traffic", "--no-cpu-baseline",
                             "--dump-outputs", str(tmp_path / d), timeout=600)
        assert rc == 0, err[-3000:]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and len(line["dump_outputs"]["files"]) == 4
        runs.append({f[:-4]: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)})
    a, b = runs
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert {k: v.dtype for k, v in a.items()} == {"encode_words": np.float64, "encode_words_index": np.float64,
                                                  "decode_bases": np.float32, "decode_bases_index": np.float64}
    words = oracle.encode(oracle.nucgen(n, seed + 2))
    assert np.array_equal(a["encode_words_index"], np.arange(words.size))
    assert np.array_equal(a["encode_words"][:, 0], (words & 0xFFFFFFFF).astype(np.float64))
    assert np.array_equal(a["encode_words"][:, 1], (words >> np.uint64(32)).astype(np.float64))
    bi = a["decode_bases_index"].astype(np.int64)
    assert bi.size == 1 << 21 and bi[0] == 0 and bi[-1] == n - 1 and bool((np.diff(bi) > 0).all())
    assert np.array_equal(a["decode_bases"], oracle.nucgen(n, seed)[bi].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_times_the_step_alone():
    """A plain one-GPU run carries the headline and the step's own per-kernel figures, and nothing that takes a run of its own: no live PMC
    pass, CPU baseline, oracle parity or side measurement; --full runs them (tests/test_gpu_comm.py)."""
    rc, lines, err = run("--gpus", "1", "--steps", "4", "--warmup", "1", "--bases", str(10**8), timeout=600)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["config"]["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["traffic"] is None and "--full" in line["roofline"]["traffic_source"]
    assert line["configs"]["cfg2_encode"] > 0 and line["configs"]["cfg2_decode"] > 0 and line["configs"]["cfg3_kmer_batch"] is None
    assert not {"cpu_baseline", "parity_vs_oracle", "shape_probe_pair", "kmer_batch", "kmer_hdist_scan", "host_path", "stream_probe_gb_s"} & line.keys()
