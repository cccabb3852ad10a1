"""The stepwise engine hands back, byte for byte, what the build recorded in tests/golden/stepwise_parent.json handed back (its commit id
is in the file): kept samples, final states, accept counts, lp where the family has it, NUTS counters and depths, the streaming
statistics.  The launch loop of lr_engine.h states each launch on an argument block it never edits, and lr_plan.h plan_stepwise decides
what the loop used to decide inline; no kernel and no argument of any launch changed, so nothing may differ.  The CPU test
tests/test_stepwise_trace_cpu.py pins which kernels are launched; this one covers what a trace cannot see -- part_f32, fuse_mid, the
number of slice partials an update sums, which buffer of a pair a launch reads.  Cases and the fixture's generator:
tests/stepwise_parent_cases.py."""
import json
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import stepwise_parent_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


@pytest.fixture(scope="module")
def recorded(la):
    with open(cases.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["recorded_from_commit"]) == 40
    # the plans scale with the chip: the recording holds for a device with as many CUs as the one it was made on
    assert cases.device_cus(la) == doc["cus"]
    return doc["cases"]


def compare(got, recorded):
    assert got, "no case ran"
    bad = []
    for cid, rec in got.items():
        want = recorded[cid]
        assert set(rec) == set(want), (cid, sorted(rec), sorted(want))
        for name, g in rec.items():
            if name == "refused":
                continue
            print(cid, name, g["shape"], g["sha256"][:16], want[name]["sha256"][:16])
            if g != want[name]:
                bad.append((cid, name, g, want[name]))
    assert not bad, bad[:4]


@pytest.mark.parametrize("dtype,n,p,opt", cases.MODELS)
def test_hmc_on_the_stepwise_engine_repeats_the_recorded_bytes(la, recorded, dtype, n, p, opt):
    """L = 1 .. 4 under the default policy (float64 models: L = 2 .. 4), precision full and bf16 at L = 4"""
    compare(cases.run_hmc_model(la, dtype, n, p, opt), recorded)


@pytest.mark.parametrize("n,p", cases.OTHER)
def test_other_families_and_closures_repeat_the_recorded_bytes(la, recorded, n, p):
    compare(cases.run_other(la, n, p), recorded)


@pytest.mark.parametrize("n,p", cases.OTHER + [cases.NUTS_TALL])
def test_stepwise_nuts_repeats_the_recorded_bytes(la, recorded, n, p):
    compare(cases.run_nuts(la, n, p), recorded)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_tall_fused_prologue_repeats_the_recorded_bytes(la, recorded, dtype):
    """1024 chains on n = 16384: the 16-wave interior kernel that finishes the previous step in its prologue (L = 3 swaps the buffer pairs
    once, L = 4 twice)"""
    compare(cases.run_tall_fused(la, dtype), recorded)


def test_statistics_and_shards_repeat_the_recorded_bytes(la, recorded):
    compare(cases.run_stats_and_shards(la), recorded)


def test_every_recorded_case_is_run(recorded):
    ids = {f"hmc-{d}-n{n}-p{p}-[{opt}]-L{L}-{prec}" for d, n, p, opt, L, prec in cases.HMC}
    ids |= {f"{k}-f32-n{n}-p{p}" for n, p in cases.OTHER for k in ("rwmh", "mala", "ul", "eval", "nuts")} | {"nuts-f32-n%d-p%d" % cases.NUTS_TALL}
    ids |= {"hmc-%s-n%d-p%d-C%d-L%d-auto" % ((d,) + cases.TALL_FUSED + (L,)) for d in ("float32", "float64") for L in (2, 3, 4)}
    ids |= {"hmc-f32-n3000-p8-L3-stats-thin2", "hmc-f32-n900-p128-[wide_traj=0]-L4-shard0", "hmc-f32-n900-p128-[wide_traj=0]-L4-shard35"}
    assert ids == set(recorded)
