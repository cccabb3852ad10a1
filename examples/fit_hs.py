#!/usr/bin/env python3
"""A sparse logistic regression under the horseshoe prior, end to end (needs an MI355X): n = 150 rows, p = 24 columns, four true effects.

Synthetic design -> model -> the horseshoe Polya-Gamma Gibbs sampler (`hsKernel`: nothing to tune, no warm-up; include/logreg_hip_hs.h)
beside the Gaussian-prior fit of the same model (`pgKernel`) -> posterior means and the horseshoe's shrinkage factors
kappa_j = 1 / (1 + tau^2 lambda_j^2): near 0 where the data speak for an effect, near 1 where the coefficient is shrunk away.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from logreg_amd import LogReg, hsKernel, mcmc, pgKernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=256)
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--burn", type=int, default=200)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()

rng = np.random.default_rng(1)
n, p = 150, 24
X = rng.standard_normal((n, p))
X[:, 0] = 1.0
truth = np.zeros(p)
truth[[1, 5, 9, 17]] = [2.0, -1.5, 1.5, -2.0]
y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ truth))).astype(np.float64)

model = LogReg(X, y, np.full(p, 5.0), dtype=a.dtype)  # N(0, 5^2) on every coefficient: the Gaussian fit's prior, the horseshoe's slab
m_shrunk, p0 = p - 1, 4  # every coordinate but the intercept is shrunk; p0 effects are expected
tau0 = p0 / (m_shrunk - p0) / np.sqrt(n)  # Piironen & Vehtari (2017): the global scale that puts p0 effective coefficients a priori
start = np.zeros((a.chains, p))
kw = dict(thin=1, iters=a.burn + a.iters, verb=False, seed=11)

gauss = mcmc(start, pgKernel(model.lpost), **kw)[a.burn:]
hs, info = mcmc(start, hsKernel(model.lpost, global_scale=tau0), return_info=True, **kw)
hs, lam2, tau2 = hs[a.burn:], info["local_scale2"][a.burn:], info["global_scale2"][a.burn:]
kappa = (1.0 / (1.0 + tau2[:, :, None] * lam2)).mean(axis=(0, 1))

print(f"global scale tau0 = {tau0:.4f}; {a.chains} chains, {a.iters} kept sweeps after {a.burn}")
print("  j   truth   Gaussian mean (sd)    horseshoe mean (sd)   kappa_j")
for j in range(p):
    g, h = gauss[:, :, j].astype(np.float64), hs[:, :, j].astype(np.float64)
    print(f" {j:2d}  {truth[j]:+5.1f}   {g.mean():+7.3f} ({g.std():.3f})     {h.mean():+7.3f} ({h.std():.3f})     " + (f"{kappa[j]:.3f}" if j else "  -  (not shrunk)"))
err = lambda b: float(np.sqrt(np.mean((b.astype(np.float64).mean(axis=(0, 1)) - truth) ** 2)))  # noqa: E731
print(f"root mean square error of the posterior mean: Gaussian {err(gauss):.3f}, horseshoe {err(hs):.3f}")
print(f"posterior median of tau: {np.sqrt(np.median(tau2)):.4f}; skipped sweeps {int(info['skipped'].sum())}, clamped draws {int(info['clamped'].sum())}")
