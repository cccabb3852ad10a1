#!/usr/bin/env python3
"""The reference's closing printout for a many-chain run that never leaves the device (needs an MI355X).

Every script of the reference ends with `scipy.stats.describe(out)` (Python/fit-np-hmc.py:113-117) and `smfsb::mcmcSummary`
(Python/analyse.R: quartiles and a histogram per coefficient) on the full sample matrix.  Here Pima HMC runs with `summary_only=True` --
no draw reaches the host -- while a `Marginals` accumulator folds every chunk of kept draws into per-coefficient histograms, min / max
and power sums.  The grid comes from `find_map`: the mode -+ 8 standard deviations of the Laplace approximation.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, Marginals, find_map, hmcKernel, load_pima, marginal_grid, mcmc  # noqa: E402
from logreg_amd.marginals import hpd, interval, quantile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--bins", type=int, default=256)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

X, y = load_pima()
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
beta, info = find_map(LogReg(X, y, pscale, dtype="float64"))
lo, hi = marginal_grid(beta, info["sd"])
pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
kern = hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre)
np.set_printoptions(linewidth=160, precision=4, suppress=True)

warm = mcmc(np.tile(beta, (a.chains, 1)), kern, thin=a.thin, iters=50, verb=False, summary_only=True, seed=1)
mg = Marginals(a.chains, model.p, a.dtype, lo, hi, bins=a.bins)
t0 = time.perf_counter()
res = mcmc(warm["state"], kern, thin=a.thin, iters=a.iters, verb=False, summary_only=True, seed=2, marginals=mg)
dt = time.perf_counter() - t0
r = res["marginals"]
print(f"{a.chains} chains x {a.iters} kept draws (thin {a.thin}) in {dt:.2f} s, accept {res['accept_rate']:.3f}, max R-hat {np.max(res['rhat']):.4f}")
print(f"DescribeResult(nobs={r['nobs']},")
print("  minmax  =", r["minmax"][0], "\n           ", r["minmax"][1])
for key in ("mean", "variance", "skewness", "kurtosis"):
    print(f"  {key:8s}=", r[key])
print(f"draws outside the grid: {int(r['underflow'].sum())} below, {int(r['overflow'].sum())} above, {int(r['nan'].sum())} NaN"
      f"   (bin width = {100 / a.bins * 16:.1f} % of the Laplace sd)")
qs = (0.025, 0.25, 0.5, 0.75, 0.975)
q = quantile(r, qs)
print("        " + "".join(f"{100 * v:>11.1f}%" for v in qs))
for j in range(model.p):
    print(f"b{j:<7d}" + "".join(f"{v:12.5f}" for v in q[:, j]))
print("95 % equal-tailed interval\n", interval(r, 0.95))
print("95 % shortest interval (to the grid's resolution)\n", hpd(r, 0.95))
print("density of b6 (every 16th bin):", r["density"][6, ::16])
mg.free()
