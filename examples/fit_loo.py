#!/usr/bin/env python3
"""WAIC and PSIS-LOO side by side without a sample matrix (needs an MI355X).

Pima, HMC (or `--nuts`) with `summary_only=True`: no draw leaves the device and neither does the [draws, rows] matrix of pointwise
log-likelihoods.  `PosteriorPredictive` sums it over the draws as they come (lppd, WAIC); `PsisLoo` keeps it on the device and reduces
it there to elpd_loo and the Pareto k-hat of every observation -- the diagnostic WAIC does not have.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, PosteriorPredictive, PsisLoo, find_map, hmcKernel, load_pima, mcmc, nutsKernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=256)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--nuts", action="store_true")
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

X, y = load_pima()
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
beta, _ = find_map(LogReg(X, y, pscale, dtype="float64"))
pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
if a.nuts:
    kern, thin = nutsKernel(model.lpost, model.glp, eps=0.05, dmm=1 / pre), 1
else:
    kern, thin = hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre), a.thin
init = np.tile(beta, (a.chains, 1))

warm = mcmc(init, kern, thin=thin, iters=50, verb=False, summary_only=True)
waic_acc = PosteriorPredictive(model)
loo_acc = PsisLoo(model, max_draws=a.chains * a.iters)   # at most 2^20 draws: the tail of an observation is sorted in on-chip memory
res = mcmc(warm["state"], kern, thin=thin, iters=a.iters, verb=False, summary_only=True, predictive=waic_acc, loo=loo_acc)
print(f"{a.chains} chains x {a.iters} kept draws, accept rate {res['accept_rate']:.3f}, max R-hat {np.max(res['rhat']):.4f}")
w, l = waic_acc.waic(), res["loo"]
print(f"WAIC : elpd_waic {w['elpd_waic']:9.3f} +- {w['se']:.3f}   p_waic {w['p_waic']:.3f}   waic  {w['waic']:.3f}")
print(f"LOO  : elpd_loo  {l['elpd_loo']:9.3f} +- {l['se']:.3f}   p_loo  {l['p_loo']:.3f}   looic {l['looic']:.3f}")
k = l["khat"]
print(f"Pareto k-hat over {len(k)} observations: {int(np.sum(k <= 0.5))} good (<= 0.5), {int(np.sum((k > 0.5) & (k <= 0.7)))} ok (<= 0.7), "
      f"{int(np.sum((k > 0.7) & (k <= 1)))} bad (<= 1), {int(np.sum(k > 1))} very bad; largest {np.max(k):.3f} at row {int(np.argmax(k))}")
print(f"smallest effective sample size of the smoothed weights: {np.min(l['n_eff']):.0f} of {l['n_draws']} draws")
worst = np.argsort(l["elpd_i"] - w["elpd_i"])[:5]
for i in worst:
    print(f"  row {i}: y = {int(y[i])}  elpd_loo {l['elpd_i'][i]:.4f}  elpd_waic {w['elpd_i'][i]:.4f}  k-hat {k[i]:.3f}")
