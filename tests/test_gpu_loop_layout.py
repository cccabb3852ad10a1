"""The straddle-free layout of the 16-lane HMC leapfrog loop (hmc_interior_rs16: the unpaired row's lone instructions in VOP3 encoding,
the reduce-scatter, prior term and kick as one aligned block -- lr_device.h group16_reduce_scatter8_kick) moves no floating-point
operation: kept samples, final states and accept counts are, byte for byte, what the parent build recorded in
tests/golden/loop_layout_parent.json computed (its commit id is in the file).  tests/test_gpu_interior_rs16.py already pins the loop at
chains 1 / 5 / 64 / 257 x L = 1 / 2 / 3 / 8 on n = 193 .. 256, MALA, RWMH and the mixed kernel against an older recording; this file adds
what that recording lacks -- cases and the fixture's generator: tests/loop_layout_cases.py.

Other callers of the changed helpers: group16_reduce_scatter8 itself is unchanged (MALA, RWMH and the mixed kernel keep it; the new
block has hmc_interior_rs16 as its only caller).  row_pairs_eval gained a template flag that only hmc_interior_rs16 sets; its other call
sites are k_chain_rs16 (in the older recording) and eval_lpost, which the older recording runs on 16 lanes only: the last test runs it
on the 32- and 64-lane register variants and through the model's value and gradient closures."""
import json
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import loop_layout_cases as cases  # noqa: E402

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
                bad.append((cid, name, g.get("hex", g["sha256"]), w.get("hex", w["sha256"])))
    assert not bad, bad[:4]


@pytest.mark.parametrize("n,C,L,rows", cases.HMC)
def test_hmc_on_16_lanes_repeats_the_parents_bytes(la, recorded, n, C, L, rows):
    """float32 HMC, precision="full", 16 lanes per chain, thin 3, 2 kept draws: the benchmark's shape at 1 / 4 / 5 chains x L = 1 / 2 / 50,
    n = 13 and 17 (one or two real rows in a lane, the rest padding), n = 250 (16 rows per lane: no unpaired row)."""
    compare(cases.run_hmc(la, n, C, L, rows), recorded)


@pytest.mark.parametrize("group,rows", cases.OTHER)
def test_other_register_variants_and_closures_repeat_the_parents_bytes(la, recorded, group, rows):
    compare(cases.run_other(la, group, rows), recorded)


def test_every_recorded_case_is_run(recorded):
    ids = {cases.hmc_id(n, C, L) for n, C, L, _ in cases.HMC} | {f"hmc-f32-n200-p8-C5-L3-group{g}" for g, _ in cases.OTHER}
    assert ids == set(recorded)
