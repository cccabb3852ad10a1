"""The CPU side of the Pima sanity bands of tests/test_gpu_adapt.py: the warm-up of include/logreg_hip_adapt.h restated by
tests/adapt_reference.py (schedule, dual averaging, pooled window variance) driving the package's generic NumPy NUTS
(logreg_amd.kernels._numpy_nuts) on the Pima model -- 64 chains, W = 300 from eps = 1 and the unit metric, then 200 sampling iterations --
for 5 seeds.  Writes tests/golden/adapt_pima_bands.json: per seed pre_j / var_golden_j and the sampling run's mean acceptance statistic,
and their spreads (the largest |ratio - 1| and |accept - delta|); the GPU test allows 2 x these.  No GPU, about ten minutes on 5 cores.

    python tools/adapt_cpu_bands.py [--seeds 5] [--chains 64] [--warmup 300] [--sample 200]

_numpy_nuts returns the new state only.  The acceptance statistic of an iteration (the mean over the tree's leaves of min(1, exp(H0 - H)))
is recomputed from what the kernel asked of the model: the wrappers record every log-posterior and gradient it evaluated, the momentum it
drew is read ahead from NumPy's generator, and the leapfrog steps are replayed with the kernel's own arithmetic."""
import argparse
import json
import multiprocessing as mp
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLDEN = os.path.join(REPO, "tests", "golden")
MAX_DEPTH, DELTA = 10, 0.8


def pima_model():
    d = json.load(open(os.path.join(GOLDEN, "pima_xy.json")))
    X, y = np.array(d["X"]), np.array(d["y"])
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    const = float(np.sum(-0.5 * np.log(2 * np.pi) - np.log(ps)))

    def lpost(b):
        with np.errstate(all="ignore"):
            return float(-np.sum(np.logaddexp(0.0, -(2 * y - 1) * (X @ b))) + const - 0.5 * np.sum(b * b / (ps * ps)))

    def glp(b):
        with np.errstate(all="ignore"):
            return X.T @ (y - 1.0 / (1.0 + np.exp(-(X @ b)))) - b / (ps * ps)
    return lpost, glp


def iteration(lpost, glp, q, eps, dmm):
    """one _numpy_nuts iteration -> (new state, acceptance statistic, leaves, divergent)"""
    from logreg_amd.kernels import _numpy_nuts
    rec_q, rec_l, rec_g = [], [], []

    def lpi(x):
        v = lpost(x)
        rec_q.append(np.array(x))
        rec_l.append(v)
        return v

    def glpi(x):
        g = glp(x)
        rec_g.append(g)
        return g
    state = np.random.get_state()
    z = np.random.randn(len(q))
    np.random.set_state(state)
    new = _numpy_nuts(lpi, glpi, eps, dmm, MAX_DEPTH)(q)
    c = 1.0 / dmm
    p0 = z * np.sqrt(dmm)
    H0 = 0.5 * np.sum(c * p0 * p0) - rec_l[0]
    ends = {-1: (q, p0, rec_g[0]), 1: (q, p0, rec_g[0])}
    k, stats, div = 1, [], False
    for d in range(MAX_DEPTH):
        if k >= len(rec_l):
            break
        sgn = 0
        for s in (1, -1):
            cq, cp, cg = ends[s]
            if np.array_equal(cq + s * eps * c * (cp + s * 0.5 * eps * cg), rec_q[k], equal_nan=True):
                sgn = s
        assert sgn != 0, "replay lost the trajectory"
        cq, cp, cg = ends[sgn]
        whole = True
        for i in range(2 ** d):
            if k >= len(rec_l):
                whole = False
                break
            cp = cp + sgn * 0.5 * eps * cg
            cq = cq + sgn * eps * c * cp
            lpl, cg = rec_l[k], rec_g[k]
            k += 1
            cp = cp + sgn * 0.5 * eps * cg
            delta = 0.5 * np.sum(c * cp * cp) - lpl - H0
            if not np.isfinite(delta) or delta > 1000:
                stats.append(0.0)
                div = True
            else:
                stats.append(1.0 if delta <= 0 else float(np.exp(-delta)))
        if whole:
            ends[sgn] = (cq, cp, cg)
    assert k == len(rec_l)
    return np.asarray(new, dtype=np.float64), float(np.mean(stats)), len(stats), div


def one_seed(args):
    seed, C, W, S = args
    import adapt_reference as ar
    lpost, glp = pima_model()
    ref = json.load(open(os.path.join(GOLDEN, "posterior_hmc.json")))["pooled"]
    mapb = np.array(json.load(open(os.path.join(GOLDEN, "map.json")))["map"])
    sd = np.array(ref["sd"])
    np.random.seed(seed)
    q = mapb + 0.5 * sd * np.random.default_rng(41).standard_normal((C, 8))
    init, ends = ar.schedule(W)
    lasts = [e - 1 for e in ends]
    starts = [init] + ends[:-1]
    eps, dmm = 1.0, np.ones(8)
    abar, draws, leaves = [], np.empty((W, C, 8)), 0
    for t in range(W):
        a = np.empty(C)
        for ch in range(C):
            q[ch], a[ch], n, _ = iteration(lpost, glp, q[ch], eps, dmm)
            leaves += n
        draws[t] = q
        abar.append(ar.abar_of(a[None])[0][0])
        da = ar.dual_averaging(abar, [r for r in lasts if r <= t], delta=DELTA)
        eps = da["next"]
        if t in lasts:
            k = lasts.index(t)
            dmm = ar.metric_of(draws[starts[k]:ends[k]], dmm)["dmm"]
    eps = da["final"]
    acc, ndiv, depth_leaves = [], 0, 0
    for t in range(S):
        for ch in range(C):
            q[ch], a1, n, dv = iteration(lpost, glp, q[ch], eps, dmm)
            acc.append(a1)
            ndiv += dv
            depth_leaves += n
    pre = 1.0 / dmm
    return {"seed": seed, "eps": eps, "pre": pre.tolist(), "ratio": (pre / sd ** 2).tolist(), "accept": float(np.mean(acc)), "divergent": int(ndiv),
            "leaves_per_iteration_warmup": leaves / (W * C), "leaves_per_iteration_sampling": depth_leaves / (S * C)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(GOLDEN, "adapt_pima_bands.json"))
    a = ap.parse_args()
    with mp.Pool(a.seeds) as pool:
        runs = pool.map(one_seed, [(1000 + s, a.chains, a.warmup, a.sample) for s in range(a.seeds)])
    ratio = np.array([r["ratio"] for r in runs])
    res = {"what": "tools/adapt_cpu_bands.py: adapt_reference.py driving logreg_amd.kernels._numpy_nuts on Pima, from eps = 1 and the unit metric",
           "chains": a.chains, "warmup": a.warmup, "sample": a.sample, "delta": DELTA, "runs": runs,
           "ratio_spread": float(np.max(np.abs(ratio - 1.0))), "accept_spread": float(max(abs(r["accept"] - DELTA) for r in runs))}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), [(r["eps"], r["accept"], r["divergent"]) for r in runs])
