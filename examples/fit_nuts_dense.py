#!/usr/bin/env python3
"""NUTS under a DENSE metric on the drop-in (needs an MI355X): what Stan calls metric=dense_e, NumPyro dense_mass=True and BlackJAX a
matrix `inverse_mass_matrix`.

Pima's covariates are not standardised, so its posterior is strongly correlated; a diagonal metric removes the scales only.  Two ways
to a full matrix:
  --metric warmup   `nuts_warmup_dense`: Stan's windows pool one p x p covariance over all chains, from eps = 1 and the unit matrix;
  --metric laplace  `laplace_metric`: the inverse Hessian at the posterior mode, no pilot run; the step size is then tuned to that
                    fixed matrix (`adapt_metric=False`).
Sampling is `mcmc` with the dense kernel, `nutsKernel(lpost, glp, eps, max_depth=, inv_metric=Sigma)`, as with any other kernel.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, find_map, laplace_metric, load_pima, mcmc, nuts_warmup_dense, print_summary, summarise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=64)
ap.add_argument("--warmup", type=int, default=1000)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--max-depth", type=int, default=10)
ap.add_argument("--metric", choices=["warmup", "laplace"], default="warmup")
ap.add_argument("--dtype", default="float32")
ap.add_argument("--seed", type=int, default=42)
a = ap.parse_args()

X, y = load_pima()
n, p = X.shape
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
start = np.zeros((a.chains, p))
if a.metric == "laplace":
    beta, _ = find_map(model)
    warm = nuts_warmup_dense(model.lpost, model.glp, start, num_warmup=a.warmup, inv_metric=laplace_metric(model, beta), adapt_metric=False,
                             max_depth=a.max_depth, seed=a.seed)
else:
    warm = nuts_warmup_dense(model.lpost, model.glp, start, num_warmup=a.warmup, max_depth=a.max_depth, seed=a.seed)
sd = np.sqrt(np.diag(warm.inv_metric))
print(f"warm-up: eps {warm.eps:.4g}, windows {warm.info['windows']} ({warm.info['metric_skipped']} refused), divergent iterations "
      f"{int(warm.info['divergent'].sum())}\ninverse metric: sd {np.round(sd, 5)}\ncorrelation\n{np.round(warm.inv_metric / np.outer(sd, sd), 2)}")
out, info = mcmc(warm.state, warm.kernel, thin=1, iters=a.iters, verb=False, seed=a.seed + 1, return_info=True)
s = summarise(out)
print("mean", s["mean"], "\nsd", s["sd"], "\nESS", np.round(s["ess"]), "\nR-hat", s.get("rhat"))
print_summary(out)
print(f"\nmean tree depth {info['mean_depth'].mean():.2f}, leapfrog steps per iteration {info['n_leapfrog'].mean() / a.iters:.1f}, "
      f"divergent {int(info['divergent'].sum())}, mean acceptance statistic {info['mean_accept_stat'].mean():.3f}")
