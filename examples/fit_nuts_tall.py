#!/usr/bin/env python3
"""NUTS on a tall model (rows off chip) through the stepwise engine: `mode="stepwise"` (needs an MI355X).

A synthetic logistic regression of `--n` rows by `--p` columns, too tall for the fused NUTS kernel (its rows do not fit the LDS; the
default mode refuses it and says so).  MAP by `find_map`, the diagonal metric from the Laplace approximation at the MAP
(`dmm = 1 / diag(laplace_metric)`: unit scales), then `nutsKernel` under `mode="stepwise"`, and the depth / divergence report.
`--p 128 --n 4096` is the wide configuration: the same call.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, find_map, laplace_metric, mcmc, nutsKernel, summarise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=8)
ap.add_argument("--chains", type=int, default=1024)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warm", type=int, default=50, help="iterations discarded before the kept ones")
ap.add_argument("--eps", type=float, default=0.5, help="step in units of the Laplace scales")
ap.add_argument("--max-depth", type=int, default=8)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

rng = np.random.default_rng(1)
X = np.column_stack([np.ones(a.n), rng.standard_normal((a.n, a.p - 1))])
beta_true = rng.standard_normal(a.p) / np.sqrt(a.p)
y = (rng.random(a.n) < 1.0 / (1.0 + np.exp(-X @ beta_true))).astype(float)
pscale = np.full(a.p, 2.0)

beta, info = find_map(LogReg(X, y, pscale, dtype="float64"))
sigma = laplace_metric(LogReg(X, y, pscale, dtype="float64"), beta)
dmm = 1.0 / np.diag(sigma)
print(f"MAP in {info['iterations']} Newton steps; Laplace scales {np.sqrt(np.diag(sigma)).min():.2e} .. {np.sqrt(np.diag(sigma)).max():.2e}")

model = LogReg(X, y, pscale, dtype=a.dtype)
kern = nutsKernel(model.lpost, model.glp, eps=a.eps, dmm=dmm, max_depth=a.max_depth)
try:
    mcmc(beta, kern, thin=1, iters=1, verb=False)
except Exception as e:  # the fused kernel's refusal names the stepwise mode
    print("default mode:", e)
start = beta + 0.5 * np.sqrt(np.diag(sigma)) * rng.standard_normal((a.chains, a.p))
out, ni = mcmc(start, kern, thin=1, iters=a.warm + a.iters, verb=False, mode="stepwise", return_info=True)
out = out[a.warm:]
s = summarise(out)
print("plan:", ni["plan"])
print("posterior mean:", np.round(s["mean"], 4))
print("true beta:     ", np.round(beta_true, 4))
print("ESS:", np.round(s["ess"]))
print(f"mean tree depth {ni['mean_depth'].mean():.2f}, leapfrog steps per draw {ni['n_leapfrog'].mean() / (a.warm + a.iters):.1f}, "
      f"divergent {int(ni['divergent'].sum())}, max-depth hits {int(ni['max_depth_hits'].sum())}, "
      f"mean acceptance statistic {ni['mean_accept_stat'].mean():.3f}")
