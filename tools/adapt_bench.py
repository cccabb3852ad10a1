#!/usr/bin/env python3
"""Cost and effect of the NUTS warm-up (include/logreg_hip_adapt.h) on Pima:
    python3 tools/adapt_bench.py [--out profiles/r18_adapt.txt] [--chains 4096] [--warmup 1000] [--repeats 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/adapt_bench.py --kernels-only --warmup 200        (for (c))

4096 chains, W = 1000, max_depth = 10, float32 and float64; times are HIP events around the enqueued sequence, the median of the repeats
with min and max beside it (one warm run first).
(a) the warm-up: W iterations x three launches, device pointers, one lr_adapt_run call, from eps = 1 and the unit metric;
(b) the same W iterations at the final (eps, dmm) from the warm-up's last state through plain lr_run_nuts: as W one-iteration launches
    and as one launch -- the difference is launch gaps; (a) against the W launches is the adaptation's own cost (its two kernels and
    the different trees of an adapting run);
(c) the two adaptation kernels per iteration: from a kernel trace of --kernels-only (the second command above; this script only runs
    the warm-up then);
(d) after the warm-up: final eps, dmm, mean tree depth and min-ESS per second of 1000 sampling iterations (Autocorr), beside the same
    run with the reference's hand-set eps = 1e-3, pre = [10, 1, 1, 1, 1, 1, 5, 1] (fit-blackjax-nuts.py:101).
Every number is recorded; none is a requirement.
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
from logreg_amd.kernels import NUTS_COUNTERS  # noqa: E402
from bench_util import Events  # noqa: E402

PRE_HAND = np.array([10.0, 1, 1, 1, 1, 1, 5, 1])


def fmt(t):
    t = np.asarray(t)
    return f"{np.median(t):.3f} s (min {t.min():.3f}, max {t.max():.3f})"


def warmup(L, model, q0, W, max_depth, ev, seed=1):
    """one device-resident warm-up -> (seconds by events, final eps, dmm, state DeviceArray, mean depth, mean accept of the last 50)"""
    Cn, p = q0.shape
    o = _lib.AdaptOpts(W=W, adapt_metric=1)
    h = C.c_void_p()
    _lib.check(L.lr_adapt_create(model.handle, Cn, C.byref(o), C.byref(h)))
    st = la.DeviceArray.from_host(model.device, np.ascontiguousarray(q0, dtype=model.np_dtype))
    cnt = la.DeviceArray(model.device, (Cn,), NUTS_COUNTERS)
    cnt.zero_()
    opts = _lib.RunOpts(n_chains=Cn, thin=1, iters=1, seed=seed, mode=_lib.MODE_AUTO, on_device=1)
    t = ev.time(lambda: _lib.check(L.lr_adapt_run(h, st.ptr, W, max_depth, C.byref(opts), None, cnt.ptr, None, None)))
    e, info = C.c_double(), _lib.AdaptInfo()
    dmm = np.empty(p)
    _lib.check(L.lr_adapt_result(h, C.byref(e), dmm.ctypes.data, C.byref(info)))
    trace = np.zeros((W, _lib.ADAPT_TRACE_COLS))
    _lib.check(L.lr_adapt_trace(h, trace.ctypes.data, None))
    L.lr_adapt_destroy(h)
    c = cnt.to_host()
    cnt.free()
    return t, e.value, dmm, st, float(c["depth_sum"].mean() / W), float(trace[-50:, 1].mean()), int(c["divergent"].sum())


def plain(L, model, st, W, per_launch, eps, dmm, max_depth, ev, seed=2):
    Ln = _lib.bind_nuts(L)
    Cn = st.shape[0]
    work = la.DeviceArray.from_host(model.device, st.to_host())
    d = np.ascontiguousarray(dmm, dtype=np.float64)

    def go():
        for i in range(W // per_launch):
            opts = _lib.RunOpts(n_chains=Cn, thin=1, iters=per_launch, iter_offset=i * per_launch, seed=seed, mode=_lib.MODE_AUTO, on_device=1)
            _lib.check(Ln.lr_run_nuts(model.handle, work.ptr, float(eps), max_depth, d.ctypes.data, C.byref(opts), None, None, None))
    t = ev.time(go)
    work.free()
    return t


def sampling(model, init, eps, dmm, iters, max_depth, label):
    kern = la.nutsKernel(model.lpost, model.glp, eps, dmm, max_depth)
    acc = la.Autocorr(init.shape[0], 8, model.np_dtype)
    acc.update(np.zeros((2, init.shape[0], 8), dtype=model.np_dtype)).reset()
    t0 = time.perf_counter()
    res = la.mcmc(init, kern, thin=1, iters=iters, verb=False, seed=3, summary_only=True, autocorr=acc)
    wall = time.perf_counter() - t0
    ess = res["autocorr"]["ess"]
    acc.free()
    return (f"{label}: eps {eps:.4g}, {iters} iterations in {wall:.2f} s wall, mean depth {np.mean(res['mean_depth']):.2f}, mean accept {np.mean(res['mean_accept_stat']):.3f}, "
            f"divergent {int(np.sum(res['divergent']))}, min ESS {ess.min():.0f} (coordinate {int(np.argmin(ess))}), min-ESS/s {ess.min() / wall:.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true", help="one warm-up per dtype and nothing else (for a kernel trace)")
    a = ap.parse_args()
    L = _lib.load_adapt()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    X, y = la.load_pima()
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    beta, info = la.find_map(la.LogReg(X, y, pscale, dtype="float64"))
    q0 = beta + 0.5 * info["sd"] * np.random.default_rng(1).standard_normal((a.chains, 8))
    ev = Events(L, 0)

    def say(s):  # (written as it comes: a run cut short keeps what it measured)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
    say(_lib.device_info(0))
    say(f"Pima, {a.chains} chains, W = {a.warmup}, max_depth = {a.max_depth}, {a.repeats} repeats after a warm run")
    for dtype in ("float32", "float64"):
        model = la.LogReg(X, y, pscale, dtype=dtype)
        runs = [warmup(L, model, q0, a.warmup, a.max_depth, ev) for _ in range(1 if a.kernels_only else a.repeats + 1)]
        t, eps, dmm, st, depth, acc, ndiv = runs[-1]
        if a.kernels_only:
            say(f"{dtype}: one warm-up, {t:.3f} s")
            continue
        ta = np.array([r[0] for r in runs[1:]])
        say(f"(a) {dtype} warm-up {fmt(ta)} = {np.median(ta) / a.warmup * 1e3:.3f} ms per iteration; final eps {eps:.5g}, pre {np.array2string(1 / dmm, precision=4)}, "
            f"mean depth over the warm-up {depth:.2f}, abar of the last 50 iterations {acc:.3f}, divergent iterations {ndiv}")
        t1 = np.array([plain(L, model, st, a.warmup, 1, eps, dmm, a.max_depth, ev) for _ in range(a.repeats + 1)][1:])
        tw = np.array([plain(L, model, st, a.warmup, a.warmup, eps, dmm, a.max_depth, ev) for _ in range(a.repeats + 1)][1:])
        say(f"(b) {dtype} plain lr_run_nuts at the final (eps, dmm): {a.warmup} one-iteration launches {fmt(t1)}, one launch {fmt(tw)}; "
            f"launch gaps {np.median(t1) - np.median(tw):.3f} s = {(np.median(t1) - np.median(tw)) / a.warmup * 1e6:.1f} us per iteration; "
            f"warm-up / launches {np.median(ta) / np.median(t1):.2f}, warm-up / one launch {np.median(ta) / np.median(tw):.2f}")
        init = st.to_host().astype(np.float64)
        say("(d) " + dtype + " " + sampling(model, init, eps, dmm, a.sample, a.max_depth, "after the warm-up (from eps = 1, unit metric)"))
        say("(d) " + dtype + " " + sampling(model, init, 1e-3, 1 / PRE_HAND, a.sample, a.max_depth, "hand-set pre = [10,1,1,1,1,1,5,1]"))
        for r in runs:
            r[3].free()
        model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
