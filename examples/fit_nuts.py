#!/usr/bin/env python3
"""The reference's Python/fit-blackjax-nuts.py, end to end, on the drop-in (needs an MI355X).

Same stages as the reference script: data block -> model closures -> MAP warm start -> NUTS with step 1e-3 and the script's
`pre` as BlackJAX's inverse mass matrix (dmm = 1 / pre here), 10 000 iterations from the MAP, no warm-up -> parquet b0..b7 ->
scipy.stats.describe-style summary.  `--chains C` runs C chains; `--eps`, `--max-depth` change the sampler.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, describe, find_map, load_pima, mcmc, nutsKernel, summarise, write_parquet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=1)
ap.add_argument("--iters", type=int, default=10000)
ap.add_argument("--eps", type=float, default=1e-3)
ap.add_argument("--max-depth", type=int, default=10)
ap.add_argument("--dtype", default="float32")
ap.add_argument("--out", default="fit-blackjax-nuts.parquet")
a = ap.parse_args()

X, y = load_pima()
n, p = X.shape
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
ll, lpost, glp = model.ll, model.lpost, model.glp

beta, _ = find_map(LogReg(X, y, pscale, dtype="float64"), np.random.randn(p) * 0.1)  # the script's gradient ascent, by Newton
print(beta)
print(ll(beta))
print(np.linalg.norm(glp(beta)))

print("Next, NUTS. Be patient...")
pre = np.array([10., 1., 1., 1., 1., 1., 5., 1.])   # blackjax.nuts(lpost, 1e-3, pre): inverse mass matrix = pre
kern = nutsKernel(lpost, glp, eps=a.eps, dmm=1 / pre, max_depth=a.max_depth)
start = beta if a.chains == 1 else np.tile(beta, (a.chains, 1))
out, info = mcmc(start, kern, thin=1, iters=a.iters, verb=False, return_info=True)
print(out)
write_parquet(out.reshape(-1, p), a.out)
print("Posterior summaries:")
summ = describe(out)                                 # scipy.stats.describe(out)
print(summ)
print("\nMean: " + str(summ["mean"]))
print("Variance: " + str(summ["variance"]))
print(f"\nmean tree depth {info['mean_depth'].mean():.2f}, leapfrog steps per draw {info['n_leapfrog'].mean() / a.iters:.0f}, "
      f"divergent {int(info['divergent'].sum())}, mean acceptance statistic {info['mean_accept_stat'].mean():.3f}")
s = summarise(out)
print("ESS:", np.round(s["ess"]), "MCSE:", s["mcse"])
