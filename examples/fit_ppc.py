#!/usr/bin/env python3
"""Posterior predictive checks of a many-chain run, without a sample matrix (needs an MI355X).

WAIC, LOO and the evidence rank models; a predictive check asks whether one model is adequate (Gelman, Meng & Stern 1996; bayesplot's
`ppc_stat_grouped`).  Pima HMC runs with `summary_only=True`, no draw leaves the device, while a `PredictiveCheck` replicates the 200
outcomes under every kept draw and counts the replicated diabetics per age group.  Then the same check on a synthetic model whose
design omits a strong two-group effect: both groups' observed counts fall in the tails of their replicates.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, PredictiveCheck, find_map, hmcKernel, load_pima, mcmc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=4096)
ap.add_argument("--iters", type=int, default=250)
ap.add_argument("--thin", type=int, default=20)
ap.add_argument("--dtype", default="float32")
a = ap.parse_args()
np.set_printoptions(linewidth=160, precision=4, suppress=True)


def table(res, names):
    print(f"  {'group':>14} {'rows':>5} {'observed':>9} {'replicated':>11} {'sd':>6} {'5 %':>5} {'95 %':>5} {'P(>=)':>7} {'P(<=)':>7} {'two-sided':>10}")
    lo, hi = res.quantile(0.05), res.quantile(0.95)
    for g, name in enumerate(names):
        flag = "  <-- misfit" if res["p_two"][g] < 0.01 else ""
        print(f"  {name:>14} {res['n_g'][g]:5d} {res['t_obs'][g]:9d} {res['mean'][g]:11.2f} {res['sd'][g]:6.2f} {lo[g]:5.0f} {hi[g]:5.0f} "
              f"{res['p_ge'][g]:7.3f} {res['p_le'][g]:7.3f} {res['p_two'][g]:10.3f}{flag}")
    print(f"  deviance: P(D_rep >= D_obs) = {res['dev_p']:.3f}; D_obs {res['dev_obs_mean']:.1f} +- {res['dev_obs_sd']:.1f}, D_rep {res['dev_rep_mean']:.1f} +- "
          f"{res['dev_rep_sd']:.1f}; {res['n']} draws, {res['n_nonfinite']} non-finite")


def run(X, y, pscale, groups, pre, eps):
    model = LogReg(X, y, pscale, dtype=a.dtype)
    beta, _ = find_map(LogReg(X, y, pscale, dtype="float64"))
    kern = hmcKernel(model.lpost, model.glp, eps=eps, l=50, dmm=1 / pre)
    warm = mcmc(np.tile(beta, (a.chains, 1)), kern, thin=a.thin, iters=50, verb=False, summary_only=True, seed=1)
    pc = PredictiveCheck(model, groups=groups, seed=2026)
    t0 = time.perf_counter()
    res = mcmc(warm["state"], kern, thin=a.thin, iters=a.iters, verb=False, summary_only=True, seed=2, check=pc)
    dt = time.perf_counter() - t0
    print(f"  {a.chains} chains x {a.iters} kept draws (thin {a.thin}) in {dt:.2f} s, accept {res['accept_rate']:.3f}: "
          f"{a.chains * a.iters * X.shape[0]:.2e} replicated outcomes")
    pc.close()
    model.close()
    return res["check"]


X, y = load_pima()
age = X[:, 7]
cuts = np.quantile(age, [0.25, 0.5, 0.75])
groups = np.searchsorted(cuts, age, side="right").astype(np.int32)
print("Pima, replicated diabetics by age quartile:")
table(run(X, y, np.array([10., 1., 1., 1., 1., 1., 1., 1.]), groups, np.array([100., 1., 1., 1., 1., 1., 25., 1.]), 1e-3),
      [f"age <= {c:.0f}" for c in cuts] + [f"age > {cuts[-1]:.0f}"])

rng = np.random.default_rng(12)
n = 300
z = (np.arange(n) % 2).astype(np.float64)
x = rng.standard_normal(n)
ys = (rng.random(n) < 1 / (1 + np.exp(-(0.4 * x + 1.5 * (2 * z - 1))))).astype(np.float64)
for name, Xs in (("design without the group (1, x)", np.stack([np.ones(n), x], axis=1)), ("design with the group (1, x, z)", np.stack([np.ones(n), x, z], axis=1))):
    print(f"synthetic, 300 rows, logit = 0.4 x +- 1.5 by group; {name}:")
    res = run(Xs, ys, np.full(Xs.shape[1], 5.0), z.astype(np.int32), np.ones(Xs.shape[1]), 5e-2)
    table(res, ["z = 0", "z = 1"])
    print("  ->", "the omitted effect is flagged" if np.all(res["p_two"] < 0.01) else "no group is flagged")
