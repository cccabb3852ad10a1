"""Cases and fixture generator of tests/test_gpu_interior_rs16.py: the kernels that share the 16-lane all-gather / reduce-scatter
helpers (lr_device.h group16_allgather_pairs, group16_reduce_scatter8) and the interior leapfrog loop hmc_interior_rs16, at the
smallest shapes where their paths differ.  Results are compared BYTE FOR BYTE with a recording made on another build:

    python tests/interior_rs16_cases.py --write tests/golden/interior_rs16_parent.json --commit <id of the recorded build's commit>

run once, on the GPU, in a checkout of that commit (this file copied into its tests/).  Every array is recorded as the SHA-256 of its
bytes (equal digests = equal bytes); arrays of up to 5 chains are recorded in full as hex as well, so that a difference can be read.
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(REPO, "tests", "golden", "interior_rs16_parent.json")
SEED, OFFSET = 20261, 7  # Philox key; chain_offset: not a multiple of 4 (a quad's four lanes share a chain's draws)
FULL_HEX_CHAINS = 5

# float32 HMC, precision="full", register variant on 16 lanes per chain.
#   n = 193, 200, 208: 13 rows per lane with 7 / 0 / 0 zero rows (193: some lanes hold a padded row; 13 is odd: the unpaired-row path)
#   n = 241, 256: 16 rows per lane, no unpaired row;  p = 5 is padded to 8
HMC_MODELS = [(n, p) for n in (193, 200, 208, 241, 256) for p in (8, 5)]
HMC_CHAINS = (1, 5, 64, 257)  # one group of a wave's four, a partial workgroup, four whole workgroups, sixteen and a tail
HMC_L = (1, 2, 3, 8)          # 0, 1, 2, 7 interior steps: none, the odd remainder alone, one unrolled trip, three trips + remainder
HMC_THIN, HMC_KEPT = 2, 3
# MALA and RWMH on k_chain_rs16<13>, and the float64 model's k_chain_mixed<13>
RS16 = [(kind, C) for kind in ("mala", "rwmh") for C in (5, 257)]
RS16_THIN, RS16_KEPT = 7, 2
MIXED = [(C, 3) for C in (5, 257)]


def data(n, p):
    """A small synthetic logistic regression, from NumPy's PCG64 streams only."""
    rng = np.random.default_rng(1000 * n + p)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    beta = rng.standard_normal(p) * 0.5
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    pscale = np.linspace(1.0, 3.0, p)  # a different prior, mass and step in every coordinate: a pair that lands in the wrong quad shows
    scale = np.linspace(0.5, 2.0, p)
    return X, y, pscale, scale


def init(n, p, C):
    return (0.3 / np.sqrt(n)) * np.random.default_rng(7 * n + 31 * p + C).standard_normal((C, p))


def record(out, info):
    rec = {}
    for name, arr in (("samples", out), ("state", info["state"]), ("accepts", info["accepts"])):
        arr = np.ascontiguousarray(arr)
        rec[name] = {"dtype": str(arr.dtype), "shape": list(arr.shape), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}
        if out.shape[1] <= FULL_HEX_CHAINS:
            rec[name]["hex"] = arr.tobytes().hex()
    return rec


def run_hmc_model(la, n, p):
    """-> {case id: record} of every (chains, L) of one float32 model"""
    X, y, pscale, scale = data(n, p)
    m = la.LogReg(X, y, pscale, dtype="float32")
    res = {}
    try:
        for C in HMC_CHAINS:
            for L in HMC_L:
                k = la.hmcKernel(m.lpost, m.glp, eps=0.5 / np.sqrt(n), l=L, dmm=scale)
                out, info = la.mcmc(init(n, p, C), k, thin=HMC_THIN, iters=HMC_KEPT, verb=False, seed=SEED, chain_offset=OFFSET,
                                    mode="reg", group=16, precision="full", return_info=True)
                assert info["plan"] == {"mode": "reg", "group": 16, "rows_per_lane": 13 if n <= 208 else 16}, info["plan"]
                res[f"hmc-f32-n{n}-p{p}-C{C}-L{L}"] = record(out, info)
    finally:
        m.close()
    return res


def run_rs16(la, kind, C):
    n, p = 200, 8
    X, y, pscale, scale = data(n, p)
    m = la.LogReg(X, y, pscale, dtype="float32")
    try:
        sc = 1.0 / np.sqrt(n)
        if kind == "mala":
            k = la.malaKernel(m.lpost, m.glp, dt=0.05 * sc * sc, pre=scale)
        else:
            k = la.mhKernel(m.lpost, la.rwProposal(0.3 * sc * scale))
        out, info = la.mcmc(init(n, p, C), k, thin=RS16_THIN, iters=RS16_KEPT, verb=False, seed=SEED, chain_offset=OFFSET,
                            mode="reg", group=16, return_info=True)
        assert info["plan"] == {"mode": "reg", "group": 16, "rows_per_lane": 13}, info["plan"]
        return {f"{kind}-f32-n{n}-p{p}-C{C}": record(out, info)}
    finally:
        m.close()


def run_mixed(la, C, L):
    n, p = 200, 8
    X, y, pscale, scale = data(n, p)
    m = la.LogReg(X, y, pscale, dtype="float64")
    try:
        k = la.hmcKernel(m.lpost, m.glp, eps=0.5 / np.sqrt(n), l=L, dmm=scale)
        out, info = la.mcmc(init(n, p, C), k, thin=HMC_THIN, iters=HMC_KEPT, verb=False, seed=SEED, chain_offset=OFFSET,
                            mode="mixed", group=16, precision="auto", return_info=True)
        assert info["plan"] == {"mode": "mixed", "group": 16, "rows_per_lane": 13}, info["plan"]
        return {f"hmc-f64-auto-n{n}-p{p}-C{C}-L{L}": record(out, info)}
    finally:
        m.close()


def run_all(la):
    res = {}
    for n, p in HMC_MODELS:
        res.update(run_hmc_model(la, n, p))
    for kind, C in RS16:
        res.update(run_rs16(la, kind, C))
    for C, L in MIXED:
        res.update(run_mixed(la, C, L))
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
