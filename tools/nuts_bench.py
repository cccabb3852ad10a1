#!/usr/bin/env python3
"""NUTS throughput and efficiency at 4096 chains (lr_nuts.h), beside HMC at the reference's l = 50, thin = 20 on the same shape:
    python3 tools/nuts_bench.py [iters]     (profiles/r7_nuts.txt is its record)

Per (data, dtype): chain-iterations/s and gradient evaluations/s of one timed launch, mean tree depth, the lockstep efficiency
sum of leapfrog steps / (4 x sum over waves of the wave's longest tree) from iterations run one launch at a time, and min-ESS/s
(batch-means ESS of the timed samples over the timed seconds) for NUTS and HMC."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402

C = 4096
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
PRE = np.array([10.0, 1, 1, 1, 1, 1, 5, 1])


def timed(cs, iters, thin):
    cs.advance(2, thin, keep=False)  # warm
    cs.sync()
    t = time.perf_counter()
    out = cs.advance(iters, thin)
    cs.sync()
    return out.to_host(), time.perf_counter() - t


def lockstep(k, q0, iters=20):
    cs = la.ChainSet(k, q0, seed=5)
    prev = cs.get_counters()["n_leapfrog"].astype(np.int64)
    used = peak = 0
    for _ in range(iters):
        cs.advance(1, 1, keep=False)
        cur = cs.get_counters()["n_leapfrog"].astype(np.int64)
        step = cur - prev
        prev = cur
        used += step.sum()
        peak += step.reshape(-1, 4).max(axis=1).sum()
    return used / (4.0 * peak)


def case(name, X, y, pscale, dmm, eps_nuts, eps_hmc, init):
    for dtype in ("float32", "float64"):
        m = la.LogReg(X, y, pscale, dtype=dtype)
        q0 = np.tile(init, (C, 1))
        k = la.nutsKernel(m.lpost, m.glp, eps=eps_nuts, dmm=dmm)
        cs = la.ChainSet(k, q0, seed=1)
        cs.advance(1, 50, keep=False)  # burn-in
        before = cs.get_counters()["n_leapfrog"].sum()
        s, dt = timed(cs, ITERS, 1)
        info = cs.get_counters()
        steps = info["n_leapfrog"].sum() - before
        # (timed() ran 2 warm iterations before the clock: count them out by the mean)
        steps_timed = steps * ITERS / (ITERS + 2)
        ess = la.summarise(s, max_chains=256)["ess"].min()
        eff = lockstep(k, cs.get_state())
        print(f"{name} {dtype} NUTS eps={eps_nuts}: {C * ITERS / dt:.3e} chain-it/s, {steps_timed / dt:.3e} grad/s, "
              f"mean depth {info['depth_sum'].sum() / (C * cs.iter_offset):.2f}, steps/it {steps / (C * (ITERS + 2)):.1f}, "
              f"lockstep efficiency {eff:.3f}, min-ESS/s {ess / dt:.3e}  ({dt:.3f} s)", flush=True)
        kh = la.hmcKernel(m.lpost, m.glp, eps=eps_hmc, l=50, dmm=dmm)
        ch = la.ChainSet(kh, q0, seed=1, precision="full")
        ch.advance(1, 1000, keep=False)
        hs, hdt = timed(ch, max(ITERS // 10, 10), 20)
        hess = la.summarise(hs, max_chains=256)["ess"].min()
        print(f"{name} {dtype} HMC l=50 thin=20 eps={eps_hmc}: {C * hs.shape[0] * 20 / hdt:.3e} chain-it/s, "
              f"{C * hs.shape[0] * 20 * 50 / hdt:.3e} grad/s, min-ESS/s {hess / hdt:.3e}  ({hdt:.3f} s)", flush=True)


X, y = la.load_pima()
mp = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
case("pima", X, y, np.array([10.0, 1, 1, 1, 1, 1, 1, 1]), 1 / PRE, 0.002, 1e-3, mp)
Xs, ys, _ = la.synthetic_logreg(200, 8)
init = la.find_map(la.LogReg(Xs, ys, np.full(8, 2.0), dtype="float64"))[0]
case("synthetic n=200 p=8", Xs, ys, np.full(8, 2.0), np.ones(8), 0.05, 0.05, init)
