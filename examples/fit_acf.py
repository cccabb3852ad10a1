#!/usr/bin/env python3
"""Geyer ESS, ESS per second and the autocorrelation function of a many-chain run, without a sample matrix (needs an MI355X).

What the reference does after a run with `smfsb::mcmcSummary` (Python/analyse.R:17-19: mean, sd, ESS, ACF plot), for every chain at once:
Pima HMC and NUTS run with `summary_only=True` -- no draw leaves the device -- while an `Autocorr` accumulator folds every chunk of kept
draws in where it is.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import Autocorr, LogReg, find_map, hmcKernel, load_pima, mcmc, nutsKernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--max-lag", type=int, default=63)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

X, y = load_pima()
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
beta, _ = find_map(LogReg(X, y, pscale, dtype="float64"))
pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
init = np.tile(beta, (a.chains, 1))
np.set_printoptions(linewidth=160, precision=3, suppress=True)

for name, kern, thin in (("HMC (eps 1e-3, L 50)", hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre), a.thin),
                         ("NUTS (eps 0.05)", nutsKernel(model.lpost, model.glp, eps=0.05, dmm=1 / pre, max_depth=8), 1)):
    warm = mcmc(init, kern, thin=thin, iters=50, verb=False, summary_only=True, seed=1)
    ac = Autocorr(a.chains, model.p, a.dtype, max_lag=a.max_lag)
    t0 = time.perf_counter()
    res = mcmc(warm["state"], kern, thin=thin, iters=a.iters, verb=False, summary_only=True, seed=2, autocorr=ac)
    dt = time.perf_counter() - t0
    r = res["autocorr"]
    print(f"\n{name}: {a.chains} chains x {a.iters} kept draws (thin {thin}) in {dt:.2f} s, accept {res['accept_rate']:.3f}, max R-hat {np.max(res['rhat']):.4f}")
    print("posterior mean        ", res["mean"])
    print("Geyer ESS (sum over chains)", np.round(r["ess"]), f"   capped series: {int(r['capped'].sum())} of {a.chains * model.p}")
    print("ESS from the pooled ACF    ", np.round(r["ess_pooled_acf"]))
    print("batch-means ESS            ", np.round(res["ess"]))
    print(f"ESS/s (smallest coordinate) {np.min(r['ess']) / dt:.3e}      MCSE {r['mcse']}")
    print("pooled ACF, lags 0..10 (rows) per coordinate (columns):")
    print(r["acf"][:11])
    ac.free()
