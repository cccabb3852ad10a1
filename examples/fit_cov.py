#!/usr/bin/env python3
"""The joint structure of the posterior for a many-chain run that never leaves the device (needs an MI355X).

The reference's analysis (`Python/analyse.R:17`) draws `image(cor(out))` from the full sample matrix, and its scripts carry a hand-set
preconditioner such as `pre = [100, 1, 1, 1, 1, 1, 25, 1]` because the coordinates of the Pima posterior differ in scale and are
correlated.  Here Pima HMC runs with `summary_only=True` -- no draw reaches the host -- while a `Covariance` accumulator folds every chunk
of kept draws into the second cross-moment and the per-chain sums.  The run prints the posterior correlation matrix and the multivariate
R-hat of Brooks & Gelman (1998), then runs again with the diagonal metric `metric(res)["dmm"]` estimated from the first run in place of
the hand-set one, and prints the smallest effective sample size of both.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import Covariance, LogReg, covariance_scaling, find_map, hmcKernel, load_pima, mcmc  # noqa: E402
from logreg_amd.covariance import metric  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

X, y = load_pima()
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
beta, info = find_map(LogReg(X, y, pscale, dtype="float64"))
center, scale = covariance_scaling(beta, info["sd"])  # the mode and the Laplace sd: only roughly right, which is all they have to be
pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
np.set_printoptions(linewidth=160, precision=3, suppress=True)


def run(dmm, eps, label):
    kern = hmcKernel(model.lpost, model.glp, eps=eps, l=50, dmm=dmm)
    warm = mcmc(np.tile(beta, (a.chains, 1)), kern, thin=a.thin, iters=50, verb=False, summary_only=True, seed=1)
    acc = Covariance(a.chains, model.p, a.dtype, center, scale)
    t0 = time.perf_counter()
    res = mcmc(warm["state"], kern, thin=a.thin, iters=a.iters, verb=False, summary_only=True, seed=2, covariance=acc)
    dt = time.perf_counter() - t0
    acc.free()
    print(f"{label}: {a.chains} chains x {a.iters} kept draws (thin {a.thin}) in {dt:.2f} s, accept {res['accept_rate']:.3f}, "
          f"max R-hat {np.max(res['rhat']):.4f}, min ESS {np.min(res['ess']):.0f}")
    return res


res = run(1 / pre, 1e-3, "hand-set metric")
r = res["covariance"]
print("posterior correlation\n", r["cor"])
print("sd", r["sd"], "\nmultivariate R-hat", round(r["rhat_mv"], 5), " per coordinate (unsplit)", np.round(r["rhat"], 5))
m = metric(r)
# the same step in units of the metric: eps scales with the geometric mean of sqrt(pre), so that eps^2 / dmm keeps its overall size
eps = 1e-3 * float(np.exp(np.mean(0.5 * np.log(pre) - 0.5 * np.log(m["pre"]))))
res2 = run(m["dmm"], eps, "estimated diagonal metric")
print(f"min ESS: hand-set {np.min(res['ess']):.0f}, estimated {np.min(res2['ess']):.0f}")
