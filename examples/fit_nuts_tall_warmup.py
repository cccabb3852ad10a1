#!/usr/bin/env python3
"""NUTS with a warm-up on a tall or wide model: `nuts_warmup_stepwise`, then `mcmc(..., mode="stepwise")` (needs an MI355X).

The model of examples/fit_nuts_tall.py -- a synthetic logistic regression of `--n` rows by `--p` columns, too tall (or, with
`--p 128 --n 4096`, too wide) for the fused NUTS kernel -- with nothing set by hand: the step size and the diagonal metric are adapted
from eps = 1 and the unit metric, pooled over all chains, as `examples/fit_nuts_warmup.py` does for Pima.  The Laplace approximation at
the MAP is computed only to print the adapted metric beside it.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, find_map, laplace_metric, mcmc, nuts_warmup, nuts_warmup_stepwise, summarise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=8)
ap.add_argument("--chains", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=1000)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--max-depth", type=int, default=8)
ap.add_argument("--dtype", default="float32")
ap.add_argument("--seed", type=int, default=42)
a = ap.parse_args()

rng = np.random.default_rng(1)
X = np.column_stack([np.ones(a.n), rng.standard_normal((a.n, a.p - 1))])
beta_true = rng.standard_normal(a.p) / np.sqrt(a.p)
y = (rng.random(a.n) < 1.0 / (1.0 + np.exp(-X @ beta_true))).astype(float)
pscale = np.full(a.p, 2.0)

model = LogReg(X, y, pscale, dtype=a.dtype)
start = np.zeros((a.chains, a.p))
try:
    nuts_warmup(model.lpost, model.glp, start, num_warmup=a.warmup, max_depth=a.max_depth, seed=a.seed)
except Exception as e:  # the fused warm-up refuses the shape
    print("default mode:", e)
warm = nuts_warmup_stepwise(model.lpost, model.glp, start, num_warmup=a.warmup, max_depth=a.max_depth, seed=a.seed)
print(f"warm-up: eps {warm.eps:.4g}, windows {warm.info['windows']}, mean tree depth {warm.info['mean_depth'].mean():.2f}, "
      f"divergent iterations {int(warm.info['divergent'].sum())}")
m64 = LogReg(X, y, pscale, dtype="float64")
beta, _ = find_map(m64)
ratio = warm.pre / np.diag(laplace_metric(m64, beta))
print(f"adapted inverse mass matrix over the Laplace variances: {ratio.min():.3f} .. {ratio.max():.3f}")
out, ni = mcmc(warm.state, warm.kernel, thin=1, iters=a.iters, verb=False, seed=a.seed + 1, mode="stepwise", return_info=True)
s = summarise(out)
print("posterior mean:", np.round(s["mean"], 4))
print("true beta:     ", np.round(beta_true, 4))
print("ESS:", np.round(s["ess"]))
print(f"mean tree depth {ni['mean_depth'].mean():.2f}, divergent {int(ni['divergent'].sum())}, mean acceptance statistic {ni['mean_accept_stat'].mean():.3f}")
