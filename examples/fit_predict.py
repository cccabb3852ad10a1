#!/usr/bin/env python3
"""Fit, criticise and predict without a sample matrix (needs an MI355X).

Pima: the first `--train` rows are the model, the rest are held out.  HMC runs with `summary_only=True` -- no draw ever leaves the
device -- while two accumulators consume every chunk of draws where it is: one on the model's own rows (in-sample lppd and WAIC), one on
the held-out rows (posterior predictive probability with its posterior sd, and the held-out log predictive density).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import ChainSet, LogReg, PosteriorPredictive, find_map, hmcKernel, load_pima, mcmc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--train", type=int, default=150)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

X, y = load_pima()
Xtr, ytr, Xte, yte = X[:a.train], y[:a.train], X[a.train:], y[a.train:]
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(Xtr, ytr, pscale, dtype=a.dtype)
beta, _ = find_map(LogReg(Xtr, ytr, pscale, dtype="float64"))
pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
kern = hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre)
init = np.tile(beta, (a.chains, 1))

# burn-in, then the kept run: every chunk of kept draws is folded into `insample` by mcmc itself ...
warm = mcmc(init, kern, thin=a.thin, iters=50, verb=False, summary_only=True)
insample = PosteriorPredictive(model)                      # the model's own rows and labels, already on the device
res = mcmc(warm["state"], kern, thin=a.thin, iters=a.iters, verb=False, summary_only=True, predictive=insample)
print(f"{a.chains} chains x {a.iters} kept draws, accept rate {res['accept_rate']:.3f}, max R-hat {np.max(res['rhat']):.4f}")
print("posterior mean:", np.round(res["mean"], 4))
w = insample.waic()
print(f"in-sample: lppd {w['lppd']:.3f}  p_waic {w['p_waic']:.3f}  elpd_waic {w['elpd_waic']:.3f} +- {w['se']:.3f}  (WAIC {w['waic']:.3f})")

# ... and any number of accumulators can be driven by hand from the device blocks of a ChainSet: the held-out rows
heldout = PosteriorPredictive(model, Xte, yte)
cs = ChainSet(kern, res["state"], seed=7)
for _ in range(4):
    block = cs.advance(max(a.iters // 20, 1), a.thin)      # DeviceArray [k, C, p]
    heldout.update(block, stream=cs.stream)
    cs.sync()
    block.free()
prob, sd = heldout.proba()
lppd = heldout.lppd()
print(f"held out ({len(yte)} rows, {heldout.n_draws} draws): log predictive density {lppd.sum():.3f} ({lppd.mean():.4f} per row), "
      f"accuracy at 0.5 {np.mean((prob > 0.5) == (yte == 1)):.3f}")
for i in range(min(8, len(yte))):
    print(f"  row {a.train + i}: y = {int(yte[i])}  P(y = 1 | x, data) = {prob[i]:.4f} +- {sd[i]:.4f}")
