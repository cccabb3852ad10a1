"""The 16-lane interior leapfrog loop and the helpers it shares with MALA / RWMH and the float64 model's mixed kernel compute, byte
for byte, what the build recorded in tests/golden/interior_rs16_parent.json computed (its commit id is in the file): kept samples,
final states and accept counts.  Changes to the all-gather, the reduce-scatter's issue order and the loop's unrolling move no
floating-point operation, so nothing may differ.  Cases and the fixture's generator: tests/interior_rs16_cases.py."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import interior_rs16_cases as cases  # noqa: E402

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
        for name in ("samples", "state", "accepts"):
            g, w = rec[name], want[name]
            print(cid, name, g["shape"], g["sha256"][:16], w["sha256"][:16])
            if (g["dtype"], g["shape"], g["sha256"]) != (w["dtype"], w["shape"], w["sha256"]) or g.get("hex") != w.get("hex"):
                bad.append((cid, name, g.get("hex", g["sha256"]), w.get("hex", w["sha256"])))
    assert not bad, bad[:4]


@pytest.mark.parametrize("n,p", cases.HMC_MODELS)
def test_hmc_interior_loop_repeats_the_recorded_bytes(la, recorded, n, p):
    """float32 HMC, precision="full", 16 lanes per chain: chains 1 / 5 / 64 / 257 x L = 1 / 2 / 3 / 8 (0, 1, 2, 7 interior steps),
    thin 2, 3 kept draws, chain_offset 7."""
    compare(cases.run_hmc_model(la, n, p), recorded)


@pytest.mark.parametrize("kind,C", cases.RS16)
def test_mala_and_rwmh_on_16_lanes_repeat_the_recorded_bytes(la, recorded, kind, C):
    compare(cases.run_rs16(la, kind, C), recorded)


@pytest.mark.parametrize("C,L", cases.MIXED)
def test_float64_model_with_float32_interior_repeats_the_recorded_bytes(la, recorded, C, L):
    compare(cases.run_mixed(la, C, L), recorded)


def test_every_recorded_case_is_run(recorded):
    ids = {f"hmc-f32-n{n}-p{p}-C{C}-L{L}" for n, p in cases.HMC_MODELS for C in cases.HMC_CHAINS for L in cases.HMC_L}
    ids |= {f"{kind}-f32-n200-p8-C{C}" for kind, C in cases.RS16} | {f"hmc-f64-auto-n200-p8-C{C}-L{L}" for C, L in cases.MIXED}
    assert ids == set(recorded)
