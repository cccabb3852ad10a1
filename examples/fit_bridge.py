#!/usr/bin/env python3
"""Variable selection by the evidence, end to end on the drop-in (needs an MI355X): the log marginal likelihood of the Pima model with
all eight columns and with one column dropped, by bridge sampling on the device, and the log Bayes factor between the two.

Per design: data block -> model -> NUTS after `nuts_warmup` -> a first half of the run gives the Gaussian proposal (`Covariance`), a
second half the bridge-sampling terms (`Bridge`, fed by `mcmc(..., bridge=)`: no sample matrix reaches the host) with the effective
sample size from `Autocorr`.  The plain Laplace approximation of log p(y) is printed beside each estimate.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import (Autocorr, Bridge, Covariance, LogReg, bridge_compare, bridge_proposal, covariance_scaling, find_map, load_pima, mcmc,  # noqa: E402
                        nuts_warmup)

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=256)
ap.add_argument("--warmup", type=int, default=500)
ap.add_argument("--iters", type=int, default=400, help="kept iterations per chain: half for the proposal, half for the terms")
ap.add_argument("--drop", type=int, default=3, help="the column left out of the smaller design")
ap.add_argument("--dtype", default="float64")
ap.add_argument("--seed", type=int, default=42)
a = ap.parse_args()

X, y = load_pima()
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])


def evidence(cols, name):
    p, half = len(cols), a.iters // 2
    model = LogReg(X[:, cols], y, pscale[cols], dtype=a.dtype)
    beta, info = find_map(model)
    laplace = info["lpost"] + 0.5 * p * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(info["hessian"])[1]
    warm = nuts_warmup(model.lpost, model.glp, np.zeros((a.chains, p)), num_warmup=a.warmup, seed=a.seed)
    center, scale = covariance_scaling(beta, info["sd"])
    cov = Covariance(a.chains, p, a.dtype, center, scale)
    first = mcmc(warm.state, warm.kernel, thin=1, iters=half, verb=False, seed=a.seed + 1, summary_only=True, covariance=cov)
    acc = Bridge(model, *bridge_proposal(first["covariance"]), max_draws=half * a.chains, seed=a.seed)
    ac = Autocorr(a.chains, p, a.dtype)
    second = mcmc(first["state"], warm.kernel, thin=1, iters=half, verb=False, seed=a.seed + 2, summary_only=True, bridge=acc, autocorr=ac)
    res = acc.result(n_eff=float(np.min(second["autocorr"]["ess"])))
    print(f"{name}: log p(y) = {res['logml']:.4f} +- {res['se']:.4f}  ({res['n_draws']} draws, effective {res['n_eff']:.0f}, {res['n_proposal']} proposal "
          f"draws, {res['iterations']} iterations)   Laplace approximation {laplace:.4f}")
    acc.close()
    model.close()
    return res


full = evidence(list(range(X.shape[1])), "all columns       ")
sub = evidence([j for j in range(X.shape[1]) if j != a.drop], f"without column {a.drop}  ")
c = bridge_compare(full, sub)
print(f"log Bayes factor, all columns against the smaller design: {c['log_bf']:+.4f} +- {c['se']:.4f}  "
      f"(posterior probability of the full design under equal prior odds: {c['prob_a']:.4f})")
