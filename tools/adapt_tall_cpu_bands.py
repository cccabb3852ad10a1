"""The CPU side of the sanity bands of tests/test_gpu_adapt_tall.py's end-to-end test, made as tools/adapt_cpu_bands.py made Pima's: the
warm-up restated by tests/adapt_reference.py driving the NumPy NUTS of tests/nuts_reference.py (the independent restatement of the sampler,
which returns an iteration's acceptance statistic with its state; its Philox stream counts the warm-up from LR_ADAPT_ITER_BASE and the
sampling run from 0, as the library does) on the tall model of
tests/golden/nuts_tall_posterior.json (n = 5001 x p = 8) -- 64 chains, W = 150 from eps = 1 and the unit metric at max_depth 6, then 200
sampling iterations -- for 5 seeds.  Writes tests/golden/adapt_tall_bands.json: per seed pre_j / var_golden_j and the sampling run's mean
acceptance statistic, and their spreads (the largest |ratio - 1| and |accept - delta|); the GPU test allows 2 x these.  No GPU.

    python tools/adapt_tall_cpu_bands.py [--seeds 5] [--chains 64] [--warmup 150] [--sample 200]
"""
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
MAX_DEPTH, DELTA = 6, 0.8


def tall_model():
    import nuts_tall_cases as ntc
    X, y, ps = ntc.POSTERIOR_MODEL()
    ps = np.broadcast_to(np.asarray(ps, dtype=np.float64), (X.shape[1],))
    const = float(np.sum(-0.5 * np.log(2 * np.pi) - np.log(ps)))

    def lpost(b):
        with np.errstate(all="ignore"):
            return float(-np.sum(np.logaddexp(0.0, -(2 * y - 1) * (X @ b))) + const - 0.5 * np.sum(b * b / (ps * ps)))

    def glp(b):
        with np.errstate(all="ignore"):
            return X.T @ (y - 1.0 / (1.0 + np.exp(-(X @ b)))) - b / (ps * ps)
    return lpost, glp


def one_seed(args):
    seed, C, W, S = args
    import adapt_reference as ar
    import nuts_reference as nr

    def iteration(x, eps, dmm, chain, it):
        t = nr.transition(lpost, glp, x, eps, dmm, MAX_DEPTH, nr.PhiloxStream(seed, chain, it, len(x)))
        return t.x, t.accept_stat, t.n_leaf, t.divergent
    lpost, glp = tall_model()
    g = json.load(open(os.path.join(GOLDEN, "nuts_tall_posterior.json")))
    sd = np.array(g["pooled"]["sd"])
    p = len(sd)
    q = np.array(g["map"]) + np.array(g["laplace_sd"]) * np.random.default_rng(41).standard_normal((C, p))
    init, ends = ar.schedule(W)
    lasts = [e - 1 for e in ends]
    starts = [init] + ends[:-1]
    eps, dmm = 1.0, np.ones(p)
    abar, draws = [], np.empty((W, C, p))
    for t in range(W):
        a = np.empty(C)
        for ch in range(C):
            q[ch], a[ch], _, _ = iteration(q[ch], eps, dmm, ch, (1 << 62) + t)
        draws[t] = q
        abar.append(ar.abar_of(a[None])[0][0])
        da = ar.dual_averaging(abar, [r for r in lasts if r <= t], delta=DELTA)
        eps = da["next"]
        if t in lasts:
            k = lasts.index(t)
            dmm = ar.metric_of(draws[starts[k]:ends[k]], dmm)["dmm"]
    eps = da["final"]
    acc, ndiv, leaves = [], 0, 0
    for t in range(S):
        for ch in range(C):
            q[ch], a1, n, dv = iteration(q[ch], eps, dmm, ch, t)
            acc.append(a1)
            ndiv += dv
            leaves += n
    pre = 1.0 / dmm
    return {"seed": seed, "eps": eps, "pre": pre.tolist(), "ratio": (pre / sd ** 2).tolist(), "accept": float(np.mean(acc)), "divergent": int(ndiv),
            "leaves_per_iteration_sampling": leaves / (S * C)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=150)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(GOLDEN, "adapt_tall_bands.json"))
    a = ap.parse_args()
    with mp.Pool(a.seeds) as pool:
        runs = pool.map(one_seed, [(1000 + s, a.chains, a.warmup, a.sample) for s in range(a.seeds)])
    ratio = np.array([r["ratio"] for r in runs])
    res = {"what": "tools/adapt_tall_cpu_bands.py: adapt_reference.py driving nuts_reference.transition on nuts_tall_cases.POSTERIOR_MODEL (5001 x 8), "
                   "from eps = 1 and the unit metric",
           "chains": a.chains, "warmup": a.warmup, "sample": a.sample, "max_depth": MAX_DEPTH, "delta": DELTA, "runs": runs,
           "ratio_spread": float(np.max(np.abs(ratio - 1.0))), "accept_spread": float(max(abs(r["accept"] - DELTA) for r in runs))}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), [(r["eps"], r["accept"], r["divergent"]) for r in runs])
