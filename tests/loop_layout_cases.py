"""Cases and fixture generator of tests/test_gpu_loop_layout.py: what tests/interior_rs16_cases.py does not reach of the code that the
straddle-free layout of the 16-lane HMC leapfrog loop touches (lr_kernels.h hmc_interior_rs16; lr_device.h row_pairs_eval's
unpaired row in VOP3 encoding, group16_reduce_scatter8_kick).  Results are compared BYTE FOR BYTE with a recording made on the
parent build:

    python tests/loop_layout_cases.py --write tests/golden/loop_layout_parent.json --commit <id of the recorded build's commit>

run once, on the GPU, in a checkout of that commit (this file and tests/interior_rs16_cases.py copied into its tests/).  Arrays are
recorded as in tests/interior_rs16_cases.py: the SHA-256 of the bytes, and the bytes themselves as hex up to 5 chains.
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (REPO, os.path.join(REPO, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import interior_rs16_cases as base  # noqa: E402  (data, init, record, SEED, OFFSET)

FIXTURE = os.path.join(REPO, "tests", "golden", "loop_layout_parent.json")
THIN, KEPT = 3, 2
# float32 HMC, precision="full", register variant on 16 lanes per chain: (n, chains, L, rows per lane)
#   n = 200: the benchmark's shape; 1 / 4 / 5 chains = a wave with three dead chains, a full wave, a second wave with three dead chains;
#            L = 1 (no interior step), 2 (one), 50 (the benchmark's 49)
#   n = 13, 17: 13 rows per lane of which 1 (lanes 0-12) or none, resp. 2 (lane 0) or 1 are real: the rest are zero padding rows
#   n = 250: 16 rows per lane, no unpaired row (the other instantiation of the 16-lane family), a padding row in lanes 10-15
HMC = [(200, C, L, 13) for C in (1, 4, 5) for L in (1, 2, 50)] + [(13, 5, 2, 13), (13, 5, 50, 13), (17, 5, 2, 13), (17, 5, 50, 13),
                                                                    (250, 5, 50, 16)]
# row_pairs_eval has one more caller than the existing recording runs: eval_lpost on the 32- and 64-lane register variants (7 and 4
# rows per lane at n = 200) -- the end points of their HMC trajectories, and the model's value / gradient closures (k_eval).
OTHER = [(32, 7), (64, 4)]


def hmc_id(n, C, L):
    return f"hmc-f32-n{n}-p8-C{C}-L{L}-thin{THIN}"


def run_hmc(la, n, C, L, rows):
    X, y, pscale, scale = base.data(n, 8)
    m = la.LogReg(X, y, pscale, dtype="float32")
    try:
        k = la.hmcKernel(m.lpost, m.glp, eps=0.5 / np.sqrt(n), l=L, dmm=scale)
        out, info = la.mcmc(base.init(n, 8, C), k, thin=THIN, iters=KEPT, verb=False, seed=base.SEED, chain_offset=base.OFFSET,
                            mode="reg", group=16, precision="full", return_info=True)
        assert info["plan"] == {"mode": "reg", "group": 16, "rows_per_lane": rows}, info["plan"]
        return {hmc_id(n, C, L): base.record(out, info)}
    finally:
        m.close()


def run_other(la, group, rows):
    """HMC on another register variant (its end points call row_pairs_eval through eval_lpost) and the closures at the same point"""
    n, C = 200, 5
    X, y, pscale, scale = base.data(n, 8)
    m = la.LogReg(X, y, pscale, dtype="float32")
    try:
        k = la.hmcKernel(m.lpost, m.glp, eps=0.5 / np.sqrt(n), l=3, dmm=scale)
        out, info = la.mcmc(base.init(n, 8, C), k, thin=THIN, iters=KEPT, verb=False, seed=base.SEED, chain_offset=base.OFFSET,
                            mode="reg", group=group, precision="full", return_info=True)
        assert info["plan"] == {"mode": "reg", "group": group, "rows_per_lane": rows}, info["plan"]
        rec = base.record(out, info)
        x0 = base.init(n, 8, C)[0]
        closures = np.concatenate([[m.lpost(x0)], np.asarray(m.glp(x0), dtype=np.float64)])
        rec["closures"] = {"dtype": str(closures.dtype), "shape": list(closures.shape),
                           "sha256": hashlib.sha256(closures.tobytes()).hexdigest(), "hex": closures.tobytes().hex()}
        return {f"hmc-f32-n{n}-p8-C{C}-L3-group{group}": rec}
    finally:
        m.close()


def run_all(la):
    res = {}
    for n, C, L, rows in HMC:
        res.update(run_hmc(la, n, C, L, rows))
    for group, rows in OTHER:
        res.update(run_other(la, group, rows))
    return res


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True)
    ap.add_argument("--commit", required=True, help="id of the commit whose build is being recorded")
    a = ap.parse_args()
    import logreg_amd
    from logreg_amd import build as lib_build
    doc = {"recorded_from_commit": a.commit, "library_build_id": lib_build.built_id(), "cases": run_all(logreg_amd)}
    os.makedirs(os.path.dirname(os.path.abspath(a.write)), exist_ok=True)
    with open(a.write, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases -> {a.write} ({os.path.getsize(a.write)} bytes)")
