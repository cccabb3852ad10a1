"""The host path of NUTS -- argument packing, metric triples, launch table, entry points and the warm-up handle, for the diagonal and
the dense metric -- hands the kernels, byte for byte, what the build recorded in tests/golden/nuts_host_parent.json handed them (its
commit id is in the file): kept samples, final states, counters and depths of fixed-metric runs; step size, metric, traces, states, draws
and counters of warm-ups.  A refactor of the host code moves no argument that reaches a kernel, so nothing may differ.  Cases and the
fixture's generator: tests/nuts_host_cases.py."""
import json
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import nuts_host_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


@pytest.fixture(scope="module")
def recorded():
    with open(cases.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["recorded_from_commit"]) == 40
    return doc["cases"]


def compare(got, recorded):
    assert got, "no case ran"
    bad = []
    for cid, rec in got.items():
        want = recorded[cid]
        assert set(rec) == set(want), (cid, sorted(rec), sorted(want))
        for name, g in rec.items():
            w = want[name]
            print(cid, name, g["shape"], g["sha256"][:16], w["sha256"][:16])
            if (g["dtype"], g["shape"], g["sha256"]) != (w["dtype"], w["shape"], w["sha256"]) or g.get("hex") != w.get("hex"):
                bad.append((cid, name, g.get("hex", g["sha256"])[:256], w.get("hex", w["sha256"])[:256]))
    assert not bad, bad[:4]


@pytest.mark.parametrize("p,dtype", cases.MODELS)
def test_fixed_metric_runs_repeat_the_recorded_bytes(la, recorded, p, dtype):
    """lr_run_nuts and lr_run_nuts_dense through ChainSet: 1 / 5 / 257 chains, max_depth 4, thin 2, 3 kept draws, chain_offset 7, a
    non-constant dmm and an inverse metric with off-diagonal terms."""
    compare(cases.run_fixed(la, p, dtype), recorded)


@pytest.mark.parametrize("p,dtype", cases.MODELS)
def test_warmups_repeat_the_recorded_bytes(la, recorded, p, dtype):
    """nuts_warmup and nuts_warmup_dense with and without metric adaptation: 40 iterations (one window, ending at 36), 5 / 257 chains,
    keep=True."""
    compare(cases.run_warmup(la, p, dtype), recorded)


def test_every_recorded_case_is_run(recorded):
    assert cases.case_ids() == set(recorded)
