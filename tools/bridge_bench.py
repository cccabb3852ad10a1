#!/usr/bin/env python3
"""Times of bridge sampling (csrc/lr_bridge.h) beside the nearest existing kernel and beside the run that feeds it:
    python3 tools/bridge_bench.py [--out FILE]      (needs the GPU; without --out the lines go to the next free profiles/rNN_bridge.txt;
                                                     they are section 2 of profiles/r27_bridge.txt)
    python3 tools/bridge_bench.py --resources       (registers and LDS of the kernels from the code objects; needs the object files, no GPU)

  terms    Bridge.update of a device-resident block (k_bridge_fill + k_bridge_gauss) per (draw, row), beside PsisLoo.update of the same
           block (k_loo_fill: the same per-pair arithmetic, stored instead of summed over the rows), at Pima (n = 200, p = 8), at
           n = 100 000 x p = 8 and at n = 4096 x p = 128, float32 and float64
  pass     one pass of the iteration over N1 = N2 = 2^20 stored terms: (time of maxit = 21 - time of maxit = 1) / 20 at tol = 0,
           host round trip included
  run      mcmc(summary_only=True) of 4096 Pima chains with and without bridge=, wall clock, and Bridge's construction (the proposal
           terms) and result
terms: a timed window is CALLS = 10 reset + update pairs enqueued back to back between two HIP events (the calls do not wait for one
another, so the launches queue up behind the kernels and the window is device time, not launch gaps), and the two accumulators take
turns, window by window, so that a drift of the clocks falls on both.  pass and run: one call a window (each synchronises inside).
One warm window, then 10 timed; the median is reported with the extremes.  What the figures cannot say: how the time of Bridge.update
divides between its two kernels, and why it differs from k_loo_fill's -- no kernel trace or counter was taken.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402

RUNS = 10
CALLS = 10  # update calls per timed window of the terms


def resources():
    from logreg_amd import build
    rows = [r for r in build.kernel_resources() if "k_bridge_" in r["name"]]
    return [f"{r['name'].split('(')[0]}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, {r['lds']} bytes of LDS, {r['scratch']} bytes of scratch" for r in rows]


def hip_timer(L, device):
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.lr_event_create(device, C.byref(a)))
    _lib.check(L.lr_event_create(device, C.byref(b)))

    def timer(fn):
        ms = C.c_float()
        _lib.check(L.lr_event_record(device, a, None))
        fn()
        _lib.check(L.lr_event_record(device, b, None))
        _lib.check(L.lr_stream_sync(device, None))
        _lib.check(L.lr_event_elapsed_ms(device, a, b, C.byref(ms)))
        return ms.value * 1e-3
    return timer


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def median_of(timer, fn):
    timer(fn)  # warm
    t = np.array([timer(fn) for _ in range(RUNS)])
    return float(np.median(t)), float(t.min()), float(t.max())


def fmt(t, unit=1e3, what="ms"):
    return f"{t[0] * unit:.3f} {what} (min {t[1] * unit:.3f}, max {t[2] * unit:.3f})"


def terms_shape(name, X, y, pscale, S, dtype, center, spread, lines):
    model = la.LogReg(X, y, pscale, dtype=dtype)
    n, p = X.shape
    rng = np.random.default_rng(1)
    B = (center[None, :] + spread * rng.standard_normal((S, p))).astype(model.np_dtype)
    dB = la.DeviceArray.from_host(model.device, B)
    ht = hip_timer(model._L, model.device)
    br = la.Bridge(model, center, np.diag(np.full(p, spread ** 2)), S, n_proposal=64)
    loo = la.PsisLoo(model, S)

    def fill_bridge():
        for _ in range(CALLS):
            br.reset()
            br.update(dB)

    def fill_loo():
        for _ in range(CALLS):
            loo.reset()
            loo.update(dB)
    ht(fill_bridge)  # warm
    ht(fill_loo)
    tb, tl = [], []
    for _ in range(RUNS):  # the two take turns
        tb.append(ht(fill_bridge) / CALLS)
        tl.append(ht(fill_loo) / CALLS)
    tb, tl = ((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in (tb, tl))
    line = (f"{name} {dtype}: S={S} n={n} p={p} | Bridge.update {fmt(tb)} = {tb[0] / (S * n) * 1e12:.2f} ps per (draw, row) | PsisLoo.update {fmt(tl)} = "
            f"{tl[0] / (S * n) * 1e12:.2f} ps per (draw, row) | bridge / loo = {tb[0] / tl[0]:.2f}")
    print(line, flush=True)
    lines.append(line)
    br.close()
    loo.close()
    dB.free()
    model.close()


def pass_time(lines):
    N = 1 << 20
    rng = np.random.default_rng(2)
    l1 = la.DeviceArray.from_host(0, -120.0 + 0.7 * rng.standard_normal(N))
    l2 = la.DeviceArray.from_host(0, -120.3 + 1.1 * rng.standard_normal(N))
    ht = hip_timer(_lib.load(), 0)
    t1 = median_of(ht, lambda: la.bridge_from_terms(l1, l2, tol=0.0, maxit=1))
    t21 = median_of(ht, lambda: la.bridge_from_terms(l1, l2, tol=0.0, maxit=21))
    res = la.bridge_from_terms(l1, l2)
    line = (f"iteration, N1 = N2 = 2^20: scan + start + 1 pass + error {fmt(t1)}; 21 passes {fmt(t21)}; per pass {(t21[0] - t1[0]) / 20 * 1e6:.1f} us "
            f"= {(t21[0] - t1[0]) / 20 / (2 * N) * 1e12:.1f} ps per term; to tol = 1e-10: {res['iterations']} iterations")
    print(line, flush=True)
    lines.append(line)
    l1.free()
    l2.free()


def whole_run(lines, chains=4096, iters=100, thin=10):
    X, y = la.load_pima()
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    for dtype in ("float32", "float64"):
        model = la.LogReg(X, y, ps, dtype=dtype)
        beta, info = la.find_map(la.LogReg(X, y, ps, dtype="float64"))
        pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
        # (every chain starts at the mode: 100 kept iterations are burnt first, so that the terms below are those of posterior draws)
        init = la.mcmc(np.tile(beta, (chains, 1)), kern, thin=thin, iters=100, verb=False, seed=2, summary_only=True)["state"]
        cov = la.laplace_metric(la.LogReg(X, y, ps, dtype="float64"), beta)
        made = []

        def make():
            for a in made:
                a.close()
            made[:] = [la.Bridge(model, beta, cov, chains * iters, seed=1)]
        tc = median_of(wall, make)
        acc = made[0]

        def with_bridge():
            acc.reset()
            la.mcmc(init, kern, thin=thin, iters=iters, verb=False, seed=3, summary_only=True, bridge=acc)
        t0 = median_of(wall, lambda: la.mcmc(init, kern, thin=thin, iters=iters, verb=False, seed=3, summary_only=True))
        t1 = median_of(wall, with_bridge)
        tr = median_of(wall, acc.result)
        res = acc.result()
        line = (f"pima {dtype}, {chains} chains x {iters} kept (thin {thin}) = {chains * iters} draws, HMC l = 20: run alone {fmt(t0)}, with bridge= {fmt(t1)} "
                f"(+{(t1[0] / t0[0] - 1) * 100:.1f} %, result() included) | Bridge(...) with {chains * iters} proposal terms {fmt(tc)} | result() {fmt(tr)} | "
                f"logml {res['logml']:.4f} +- {res['se']:.1e} (n_eff = the number of draws: the error is understated), {res['iterations']} iterations")
        print(line, flush=True)
        lines.append(line)
        acc.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the lines to this file (default: the next free profiles/rNN_bridge.txt)")
    ap.add_argument("--scale", type=int, default=1, help="divide the draw and row counts (a quick look)")
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers and LDS from the code objects and exit")
    a = ap.parse_args()
    if a.resources:
        print("\n".join(resources()))
        return 0
    lines = [_lib.device_info(0), f"median of {RUNS} windows after a warm one ({CALLS} update calls a window for the terms)"]
    print(lines[0], flush=True)
    X, y = la.load_pima()
    mp = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    Xt, yt, bt = la.synthetic_logreg(100000 // a.scale, 8)
    Xw, yw, bw = la.synthetic_logreg(4096 // a.scale, 128)
    for dtype in ("float32", "float64"):
        terms_shape("pima", X, y, ps, 4096 * 64 // a.scale, dtype, mp, 0.02, lines)
        terms_shape("tall", Xt, yt, np.ones(8), 4096, dtype, bt, 0.02, lines)
        terms_shape("wide", Xw, yw, np.ones(128), 4096, dtype, bw, 0.02, lines)
    pass_time(lines)
    whole_run(lines, chains=4096 // a.scale)
    if not a.out:
        import re
        taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(REPO, "profiles"))) if m]
        a.out = os.path.join(REPO, "profiles", f"r{max(taken, default=0) + 1}_bridge.txt")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
