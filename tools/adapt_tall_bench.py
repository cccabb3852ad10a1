#!/usr/bin/env python3
"""The NUTS warm-up on the stepwise engine, measured (needs an MI355X): python tools/adapt_tall_bench.py [--out FILE]

The two shapes of profiles/r23_nuts_tall.txt -- n = 100 000 x p = 8 (tall) and n = 4096 x p = 128 (wide), synthetic, float32 -- at 1024 chains.
Per shape:

* W = 1000 warm-up iterations from eps = 1 and the unit metric (`nuts_warmup_stepwise`): HIP events around the call on the
  stream it runs on, and wall time;
* beside it 1000 iterations of plain stepwise NUTS at the final tuning from the warmed-up states: what the same number of iterations costs
  without the adaptation launches (not the same trees: the warm-up's first iterations run at other step sizes);
* 1000 sampling iterations after the warm-up: mean depth, mean acceptance statistic, min-ESS (of the first 128 chains' draws) per second of the whole run; beside it the same run at the
  hand-set tuning of r23 (the Laplace-scale diagonal metric, step 0.5).

The share of the two adaptation kernels in the warm-up's time needs a kernel trace, taken in a run of its own (`--short`: W = 200 and no
sampling runs, for `rocprofv3 --kernel-trace --stats -- python tools/adapt_tall_bench.py --short`).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--chains", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=1000)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--max-depth", type=int, default=8)
ap.add_argument("--short", action="store_true")
a = ap.parse_args()
if a.short:
    a.warmup = 200

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def problem(n, p):  # tools/nuts_tall_bench.py's
    rng = np.random.default_rng(1)
    X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
    beta = rng.standard_normal(p) / np.sqrt(p)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    return X, y, np.full(p, 2.0)


class Events:
    """milliseconds between two events on the NULL stream, where calls made with host pointers run"""

    def __init__(self, device):
        self.L, self.dev = _lib.load(), device
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            _lib.check(self.L.lr_event_create(device, C.byref(e)))

    def __enter__(self):
        _lib.check(self.L.lr_event_record(self.dev, self.e[0], None))
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        _lib.check(self.L.lr_event_record(self.dev, self.e[1], None))
        _lib.check(self.L.lr_stream_sync(self.dev, None))
        self.wall = time.perf_counter() - self.t0
        ms = C.c_float()
        _lib.check(self.L.lr_event_elapsed_ms(self.dev, self.e[0], self.e[1], C.byref(ms)))
        self.ms = float(ms.value)


ESS_CHAINS = 128  # the effective sample size is computed on the host from the first chains' draws; the time is the whole run's


def sample(kernel, state, iters, ev):
    cs = la.ChainSet(kernel, np.ascontiguousarray(state), seed=3, mode="stepwise")
    with ev:
        d = cs.advance(iters, 1)
        cs.sync()
    out, info = d.to_host(), cs.nuts_info()
    ess = la.summarise(out[:, :ESS_CHAINS].astype(np.float64))["ess"]
    return dict(ms=ev.ms, wall=ev.wall, depth=float(np.mean(info["mean_depth"])), accept=float(np.mean(info["mean_accept_stat"])), div=int(info["divergent"].sum()),
                min_ess=float(np.min(ess)), state=out[-1])


say(f"NUTS warm-up on the stepwise engine (nuts_warmup_stepwise), float32, {a.chains} chains, W = {a.warmup} from eps = 1 and the unit metric, max_depth {a.max_depth}")
for n, p in ((100000, 8), (4096, 128)):
    X, y, ps = problem(n, p)
    m64 = la.LogReg(X, y, ps, dtype="float64")
    beta, _ = la.find_map(m64)
    sd = np.sqrt(np.diag(la.laplace_metric(m64, beta)))
    m = la.LogReg(X, y, ps, dtype="float32")
    ev = Events(m.device)
    q0 = beta + 0.5 * sd * np.random.default_rng(2).standard_normal((a.chains, p))
    la.nuts_warmup_stepwise(m.lpost, m.glp, q0, 5, max_depth=a.max_depth, seed=1)  # the first-launch costs, the workspace
    with ev:
        res = la.nuts_warmup_stepwise(m.lpost, m.glp, q0, a.warmup, max_depth=a.max_depth, seed=1)
    leaps = int(res.info["n_leapfrog"].sum())
    say(f"n={n} p={p}: warm-up {ev.ms:.1f} ms by HIP events, {1e3 * ev.wall:.1f} ms wall ({ev.ms / a.warmup:.3f} ms per iteration); eps {res.eps:.4g}, windows {res.info['windows']}, "
        f"metric_skipped {res.info['metric_skipped']}, mean depth over the warm-up {float(np.mean(res.info['mean_depth'])):.2f}, {leaps} chain leapfrog steps, "
        f"divergent iterations {int(res.info['divergent'].sum())}; pre / Laplace variance min {float(np.min(res.pre / sd ** 2)):.3f} max {float(np.max(res.pre / sd ** 2)):.3f}")
    if a.short:
        continue
    plain = sample(res.kernel, res.state, a.warmup, ev)
    say(f"    {a.warmup} plain stepwise iterations at the final tuning: {plain['ms']:.1f} ms by HIP events, {1e3 * plain['wall']:.1f} ms wall ({plain['ms'] / a.warmup:.3f} ms per iteration), "
        f"mean depth {plain['depth']:.2f}")
    tuned = sample(res.kernel, plain["state"], a.iters, ev)
    hand = la.nutsKernel(m.lpost, m.glp, eps=0.5, dmm=1 / sd ** 2, max_depth=a.max_depth)
    hs = sample(hand, sample(hand, q0, 50, ev)["state"], a.iters, ev)
    for name, r in (("adapted", tuned), ("hand-set (Laplace-scale metric, step 0.5)", hs)):
        say(f"    {a.iters} sampling iterations, {name}: mean depth {r['depth']:.2f}, accept stat {r['accept']:.3f}, divergent {r['div']}, min ESS {r['min_ess']:.0f} over the first "
            f"{min(ESS_CHAINS, a.chains)} chains, {r['wall']:.2f} s wall -> min-ESS/s {r['min_ess'] / r['wall']:.4g}")
say("the two adaptation kernels' share of the warm-up's time: from a kernel trace of a run of its own (--short), where one was taken")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
