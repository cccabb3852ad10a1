#!/usr/bin/env python3
"""Rank-normalised split-R-hat, bulk-ESS and tail-ESS of a many-chain run, without a sample matrix (needs an MI355X).

The convergence report of Stan, ArviZ and R's `posterior` (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021) -- "R-hat < 1.01, bulk and
tail ESS are N" -- for thousands of chains at once: Pima HMC runs with `summary_only=True`, no draw leaves the device, while a
`RankDiagnostics` accumulator keeps every chunk of kept draws where it is and ranks them when the run is over.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, RankDiagnostics, find_map, hmcKernel, load_pima, mcmc  # noqa: E402

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
np.set_printoptions(linewidth=160, precision=4, suppress=True)

kern = hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre)
warm = mcmc(init, kern, thin=a.thin, iters=50, verb=False, summary_only=True, seed=1)
rk = RankDiagnostics(a.chains, model.p, a.iters, a.dtype, max_lag=a.max_lag)
t0 = time.perf_counter()
res = mcmc(warm["state"], kern, thin=a.thin, iters=a.iters, verb=False, summary_only=True, seed=2, rank=rk)
dt = time.perf_counter() - t0
r = res["rank"]
print(f"HMC (eps 1e-3, L 50): {a.chains} chains x {a.iters} kept draws (thin {a.thin}) in {dt:.2f} s, accept {res['accept_rate']:.3f}")
print("posterior mean              ", res["mean"])
print("median (exact)              ", r["median"])
print("5 % and 95 % order statistic", r["q05"], r["q95"])
print("classical split-R-hat       ", res["rhat"])
print("rank-normalised R-hat: bulk ", r["rhat_bulk"])
print("                     folded ", r["rhat_tail"])
print("bulk-ESS                    ", np.round(r["ess_bulk"]), f"  capped: {int(np.nansum(r['capped_bulk']))} of {model.p}")
print("tail-ESS                    ", np.round(r["ess_tail"]))
print("batch-means ESS             ", np.round(res["ess"]))
print(f"R-hat < 1.01: {bool(np.all(r['rhat'] < 1.01))}; smallest bulk-ESS / s {np.min(r['ess_bulk']) / dt:.3e}, smallest tail-ESS / s {np.min(r['ess_tail']) / dt:.3e}")
# the rank histogram of chain 0 in coordinate 0 (20 bins): flat when the chain explores what the others do
twice_r = rk.ranks(0)
S = twice_r.size
print("rank histogram of chain 0   ", np.histogram(twice_r[:, 0] / (2.0 * S), bins=20, range=(0.0, 1.0))[0])
rk.free()
model.close()
