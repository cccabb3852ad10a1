#!/usr/bin/env python3
"""NUTS on the stepwise engine, measured (needs an MI355X): python tools/nuts_tall_bench.py [--out profiles/r23_nuts_tall.txt]

Two models -- n = 100 000 x p = 8 (tall) and n = 4096 x p = 128 (wide), synthetic, float32 -- at 1024 and 4096 chains, the diagonal metric of
the Laplace approximation at the MAP, step 0.5 in its units.  Per configuration:

* leapfrog steps per second: the sum of n_leapfrog over the wall time of the call, which ends in a synchronise;
* lockstep efficiency: the sum of n_leapfrog over C x the steps launched.  An iteration launches 2^D - 1 steps, D the largest depth
  among its chains (the host stops at the end of the doubling after which no chain is building), so the steps launched are read off the
  depths of the run;
* microseconds per launched step (one evaluation + one update launch), beside the stepwise HMC's microseconds per evaluation at
  precision="full" on the same model in the same process, the two alternated `--reps` times (medians).

Not measured here: the share of time the host spends waiting on the tally (it needs a kernel trace, taken in a run of its own).
The CPU measurements behind the test bounds (tests/nuts_tall_cases.py) are appended by hand below the figures.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import logreg_amd as la  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-depth", type=int, default=8)
a = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def problem(n, p):
    rng = np.random.default_rng(1)
    X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
    beta = rng.standard_normal(p) / np.sqrt(p)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    return X, y, np.full(p, 2.0)


say(f"NUTS on the stepwise engine (mode=\"stepwise\"), float32, max_depth {a.max_depth}, {a.iters} iterations per call, medians of {a.reps} alternated calls")
for n, p in ((100000, 8), (4096, 128)):
    X, y, ps = problem(n, p)
    m64 = la.LogReg(X, y, ps, dtype="float64")
    beta, _ = la.find_map(m64)
    sd = np.sqrt(np.diag(la.laplace_metric(m64, beta)))
    m = la.LogReg(X, y, ps, dtype="float32")
    nuts = la.nutsKernel(m.lpost, m.glp, eps=0.5, dmm=1 / sd ** 2, max_depth=a.max_depth)
    L = 8
    hmc = la.hmcKernel(m.lpost, m.glp, eps=0.3, l=L, dmm=1 / sd ** 2)
    for C in (1024, 4096):
        q0 = beta + 0.5 * sd * np.random.default_rng(2).standard_normal((C, p))
        cn = la.ChainSet(nuts, q0, seed=1, mode="stepwise")
        ch = la.ChainSet(hmc, q0, seed=1, mode="stepwise", precision="full")
        cn.advance(5, 1, keep=False)  # away from the start, and the first-launch costs
        ch.advance(5, 1, keep=False)
        cn.sync(); ch.sync()
        t_n, t_h, leap, steps = [], [], [], []
        for _ in range(a.reps):
            d = la.DeviceArray(m.device, (a.iters, C), np.int8)
            before = cn.get_counters()["n_leapfrog"].sum()
            t0 = time.perf_counter()
            cn.advance(a.iters, 1, keep=False, depth=d)
            cn.sync()
            t_n.append(time.perf_counter() - t0)
            leap.append(int(cn.get_counters()["n_leapfrog"].sum() - before))
            steps.append(int((2 ** np.abs(d.to_host().astype(np.int64)).max(axis=1) - 1).sum()))
            t0 = time.perf_counter()
            ch.advance(a.iters, 1, keep=False)
            ch.sync()
            t_h.append(time.perf_counter() - t0)
        i = int(np.argsort(t_n)[len(t_n) // 2])
        info = cn.nuts_info()
        say(f"n={n} p={p} chains={C} plan {cn.plan()}: {leap[i] / t_n[i]:.4g} leapfrog steps/s; lockstep efficiency {leap[i] / (C * steps[i]):.3f} "
            f"({leap[i]} chain steps in {steps[i]} launched steps x {C}); {1e6 * t_n[i] / steps[i]:.1f} us per launched step | stepwise HMC (L={L}, full) "
            f"{1e6 * float(np.median(t_h)) / (a.iters * L):.1f} us per evaluation; mean depth {info['mean_depth'].mean():.2f}, accept stat "
            f"{info['mean_accept_stat'].mean():.3f}, divergent {int(info['divergent'].sum())}")
say("not measured: the share of time in host waits (no kernel trace was taken)")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
