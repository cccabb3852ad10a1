#!/usr/bin/env python3
"""The role of the reference's R/fit-rjags.R -- a Gibbs sampler with nothing to tune -- end to end on the drop-in (needs an MI355X).

Data block -> model -> MAP start -> the Polya-Gamma Gibbs sampler (`pgKernel`: no step size, no proposal scale, no mass matrix, no
warm-up; include/logreg_hip_pg.h), thin 10 as the JAGS script -> parquet b0..b7 -> summary, with the reference's HMC posterior
(tests/golden/posterior_hmc.json, where the repository is at hand) beside it.  `--chains C` runs C chains.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from logreg_amd import LogReg, describe, find_map, load_pima, mcmc, pgKernel, summarise, write_parquet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=64)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--thin", type=int, default=10)
ap.add_argument("--dtype", default="float32")
ap.add_argument("--out", default="fit-pg.parquet")
a = ap.parse_args()

X, y = load_pima()
n, p = X.shape
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)
beta, _ = find_map(LogReg(X, y, pscale, dtype="float64"), np.random.randn(p) * 0.1)
print(beta)

kern = pgKernel(model.lpost)  # nothing to set
start = beta if a.chains == 1 else np.tile(beta, (a.chains, 1))
out, info = mcmc(start, kern, thin=a.thin, iters=a.iters, verb=False, return_info=True)
write_parquet(out.reshape(-1, p), a.out)
print("Posterior summaries:")
summ = describe(out)
print("Mean:     " + str(summ["mean"]))
print("Variance: " + str(summ["variance"]))
golden = os.path.join(ROOT, "tests", "golden", "posterior_hmc.json")
if os.path.exists(golden):
    with open(golden) as f:
        ref = json.load(f)["pooled"]
    print("reference HMC mean: " + str(np.array(ref["mean"])))
    print("reference HMC var:  " + str(np.array(ref["sd"]) ** 2))
print(f"\nproposals per draw {info['proposals_per_draw'].mean():.5f} (theory <= 1.0009), series terms per draw "
      f"{info['series_terms_per_draw'].mean():.4f}, skipped iterations {int(info['skipped'].sum())}")
if out.ndim == 3:
    s = summarise(out)
    print("ESS:", np.round(s["ess"]), "MCSE:", s["mcse"])
