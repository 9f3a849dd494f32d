"""The argument sweep over the 56 searches along a reference (tests/kmer_ref_args.py) against its recorded results (tests/golden/kmer_ref_args.json):
every single argument fault and every pair of faults on different arguments, per case the status, err's value / index / byte and which outputs still
hold the sentinel.  Every comparison is exact.  The host forms run here, through a NULL context below the host cutoff; the asynchronous forms run on a
device (-m gpu).  The plan itself is checked first: the 56 symbols against the header, the constants, the fixture's case lists against the plan's."""
import os
import re

import pytest

import kmer_ref_args as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = [e for e in ra.ENTRIES if e.host]
ASYNC = [e for e in ra.ENTRIES if not e.host]


@pytest.fixture(scope="module")
def lib():
    from bitnuc_amd import _lib as L, build
    build.ensure_built()
    return L.load()


@pytest.fixture(scope="module")
def fixture():
    return ra.load_fixture()


def test_plan_covers_the_56_entry_points_of_the_header(fixture):
    header = open(os.path.join(ROOT, "include", "bitnuc_hip.h")).read()
    declared = set(re.findall(r"\b(bitnuc_kmer_[a-z0-9_]+)\s*\(", header))
    mine = {e.symbol for e in ra.ENTRIES}
    assert len(ra.ENTRIES) == len(mine) == 56 and len(HOST) == len(ASYNC) == 28 and mine <= declared
    # what the header declares besides: the single-query scan and the fused count, whose host forms are pipelines
    assert declared - mine == {"bitnuc_kmer_hdist_" + s + t for s in ("scan", "count") for t in ("_dev", "_packed_dev", "_packed")} | {"bitnuc_kmer_hdist_scan"}
    assert f"#define BITNUC_MAX_QUERIES {ra.MAX_QUERIES}\n" in header and f"#define BITNUC_HIST_MAX_BINS {ra.HIST_MAX_BINS}\n" in header
    assert set(fixture) == mine
    for e in ra.ENTRIES:
        cases = ra.cases(e)
        labels = [c[0] for c in cases]
        assert len(set(labels)) == len(labels) and fixture[e.symbol]["labels"] == ra.labels_digest(e) and len(fixture[e.symbol]["cases"]) == len(cases)
        singles = {label for label, _ in ra.faults(e)}
        assert {"k=0", "k=33", "n=k-1", "data=NULL", "data+1"} <= singles and ("n_words-1" in singles) == e.packed == ("data+4" in singles)
        assert ("cap=0,pos=NULL" in singles) == (e.family == "hits") and ("bins=0" in singles) == (e.family == "hist")
        assert ("query=NULL" in singles) == (e.family == "hits" and e.pattern) and ("queries+4" in singles) == (e.family != "hits" and not e.pattern)
        nf = len(singles)
        assert nf * (nf - 1) // 2 >= len(cases) - 1 - nf > nf * (nf - 1) // 2 - 3 * nf  # every pair but those on one argument
    assert os.path.getsize(ra.FIXTURE) < 200_000


def _compare(e, got, fixture):
    want = ra.unpack(fixture[e.symbol])
    diff = [(label, w, g) for (label, _), w, g in zip(ra.cases(e), want, got) if w != g]
    assert not diff, f"{e.symbol}: {len(diff)} of {len(want)} cases differ; (case, recorded, got) of the first: {diff[:5]}"
    assert got[0][0] == 0 and got[0][4] & (1 << (len(ra.OUTPUTS[e.family]) - 1)) == 0  # the base call succeeds and writes its last output


@pytest.mark.parametrize("e", HOST, ids=[e.symbol for e in HOST])
def test_host_forms_answer_every_fault_and_pair_as_recorded(e, lib, fixture):
    _compare(e, ra.run(e, lib), fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("e", ASYNC, ids=[e.symbol for e in ASYNC])
def test_async_forms_answer_every_fault_and_pair_as_recorded(e, lib, ctx, fixture):
    _compare(e, ra.run(e, lib, ctx._h), fixture)
