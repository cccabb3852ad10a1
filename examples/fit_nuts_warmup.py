#!/usr/bin/env python3
"""The reference's Python/fit-numpyro.py, end to end, on the drop-in (needs an MI355X).

Same stages as the reference script: data block -> model -> NUTS with 1000 warm-up iterations (`MCMC(kernel, num_warmup=1000, ...)`,
fit-numpyro.py:44) and 10 000 samples at thin 1 -> summary -> parquet b0..b7 -> scipy.stats.describe-style summary.  The warm-up is
`nuts_warmup`: Stan-style windowed adaptation of the step size and the diagonal metric from eps = 1 and the unit metric, nothing set by
hand.  NumPyro starts from a random point; this script starts from zeros.  `--chains C` runs (and pools the adaptation over) C chains.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from logreg_amd import LogReg, load_pima, mcmc, nuts_warmup, print_summary, summarise, write_parquet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=1)
ap.add_argument("--warmup", type=int, default=1000)
ap.add_argument("--iters", type=int, default=10000)
ap.add_argument("--max-depth", type=int, default=10)
ap.add_argument("--dtype", default="float32")
ap.add_argument("--seed", type=int, default=42)
ap.add_argument("--out", default="fit-numpyro.parquet")
a = ap.parse_args()

X, y = load_pima()
n, p = X.shape
pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
model = LogReg(X, y, pscale, dtype=a.dtype)

print("Running MCMC now...")
start = np.zeros((a.chains, p))
warm = nuts_warmup(model.lpost, model.glp, start, num_warmup=a.warmup, max_depth=a.max_depth, seed=a.seed)
print(f"warm-up: eps {warm.eps:.4g}, inverse mass matrix {np.round(warm.pre, 5)}, mean tree depth {warm.info['mean_depth'].mean():.2f}, "
      f"divergent iterations {int(warm.info['divergent'].sum())}, windows {warm.info['windows']}")
out, info = mcmc(warm.state if a.chains > 1 else warm.state[0], warm.kernel, thin=1, iters=a.iters, verb=False, seed=a.seed + 1, return_info=True)
print("MCMC finished.")
s = summarise(out)                                   # mcmc.print_summary(): mean, sd, ESS, R-hat
print("mean", s["mean"], "\nsd", s["sd"], "\nESS", np.round(s["ess"]), "\nR-hat", s.get("rhat"))
print(out)
write_parquet(out.reshape(-1, p), a.out)
print_summary(out)                                   # scipy.stats.describe(out), Mean, Variance
print(f"\nmean tree depth {info['mean_depth'].mean():.2f}, divergent {int(info['divergent'].sum())}, mean acceptance statistic {info['mean_accept_stat'].mean():.3f}")
