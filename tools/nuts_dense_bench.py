#!/usr/bin/env python3
"""Cost and effect of the dense NUTS metric (include/logreg_hip_dense.h) on Pima:
    python3 tools/nuts_dense_bench.py [--out profiles/r19_nuts_dense.txt] [--chains 4096] [--warmup 1000] [--sample 1000] [--repeats 5]

4096 chains, max_depth = 10, float32 and float64; times are HIP events around the enqueued launches, the median of the repeats after a
warm run, with min and max beside it; the two kernels of a comparison alternate inside one process.
(a) the cost of the matrix products alone: k_nuts_dense against k_nuts at the same eps and a DIAGONAL Sigma = diag(1 / dmm) (the same
    trees, leaf for leaf): seconds per launch, leapfrog steps from the counters, picoseconds per leapfrog step and chain;
(b) after a W-iteration warm-up from eps = 1 and the unit metric, dense against diagonal: eps, mean depth, leapfrog steps per iteration,
    seconds per `sample` sampling iterations (events), min-ESS per second (Autocorr);
(c) registers, LDS and occupancy of the sixteen k_nuts_dense kernels (logreg_amd.build.kernel_resources: read from the code objects).
Every number is recorded; none is a requirement.  No GPU: the script fails, it does not fall back.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402
from logreg_amd.kernels import NUTS_COUNTERS  # noqa: E402
from bench_util import Events  # noqa: E402


def fmt(t):
    t = np.asarray(t)
    return f"{np.median(t):.4f} s (min {t.min():.4f}, max {t.max():.4f})"


def launch(L, model, st0, iters, eps, max_depth, ev, *, dmm=None, sigma=None, seed=2):
    """one launch of `iters` iterations from st0 (host) -> (seconds, leapfrog steps summed over the chains, depth sum)"""
    Cn = st0.shape[0]
    work = la.DeviceArray.from_host(model.device, st0)
    cnt = la.DeviceArray(model.device, (Cn,), NUTS_COUNTERS)
    cnt.zero_()
    opts = _lib.RunOpts(n_chains=Cn, thin=1, iters=iters, seed=seed, mode=_lib.MODE_AUTO, on_device=1)
    if sigma is not None:
        s = np.ascontiguousarray(sigma, dtype=np.float64)
        go = lambda: _lib.check(L.lr_run_nuts_dense(model.handle, work.ptr, float(eps), max_depth, s.ctypes.data, C.byref(opts), None, cnt.ptr, None))  # noqa: E731
    else:
        d = np.ascontiguousarray(dmm, dtype=np.float64)
        go = lambda: _lib.check(L.lr_run_nuts(model.handle, work.ptr, float(eps), max_depth, d.ctypes.data, C.byref(opts), None, cnt.ptr, None))  # noqa: E731
    t = ev.time(go)
    c = cnt.to_host()
    work.free()
    cnt.free()
    return t, int(c["n_leapfrog"].sum()), int(c["depth_sum"].sum())


def ess_run(model, init, kern, iters):
    acc = la.Autocorr(init.shape[0], 8, model.np_dtype)
    acc.update(np.zeros((2, init.shape[0], 8), dtype=model.np_dtype)).reset()
    res = la.mcmc(init, kern, thin=1, iters=iters, verb=False, seed=3, summary_only=True, autocorr=acc)
    ess = res["autocorr"]["ess"]
    acc.free()
    return float(ess.min()), int(np.argmin(ess)), float(np.mean(res["mean_accept_stat"])), int(np.sum(res["divergent"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-depth", type=int, default=10)
    a = ap.parse_args()
    _lib.require_gpu()
    L = _lib.bind_dense(_lib.load_nuts())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def say(s):  # (written as it comes: a run cut short keeps what it measured)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
    X, y = la.load_pima()
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    beta, info = la.find_map(la.LogReg(X, y, pscale, dtype="float64"))
    q0 = beta + 0.5 * info["sd"] * np.random.default_rng(1).standard_normal((a.chains, 8))
    ev = Events(L, 0)
    say(_lib.device_info(0))
    say(f"Pima, {a.chains} chains, W = {a.warmup}, {a.sample} sampling iterations, max_depth = {a.max_depth}, medians of {a.repeats} after a warm run")
    for dtype in ("float32", "float64"):
        model = la.LogReg(X, y, pscale, dtype=dtype)
        diag = la.nuts_warmup(model.lpost, model.glp, q0, a.warmup, max_depth=a.max_depth, seed=1)
        dense = la.nuts_warmup_dense(model.lpost, model.glp, q0, a.warmup, max_depth=a.max_depth, seed=1)
        st_diag, st_dense = diag.state.astype(model.np_dtype), dense.state.astype(model.np_dtype)
        # (a) the same trees through both kernels: the diagonal run's (eps, dmm), the dense kernel at Sigma = diag(1 / dmm)
        iters_a = max(1, a.sample // 10)
        td, tn = [], []
        for r in range(a.repeats + 1):
            t1, leap1, _ = launch(L, model, st_diag, iters_a, diag.eps, a.max_depth, ev, dmm=diag.dmm)
            t2, leap2, _ = launch(L, model, st_diag, iters_a, diag.eps, a.max_depth, ev, sigma=np.diag(1.0 / diag.dmm))
            if r:
                td.append(t1)
                tn.append(t2)
        per = lambda t, leap: np.median(t) / leap * 1e12  # noqa: E731
        say(f"(a) {dtype} {iters_a} iterations at eps {diag.eps:.4g} and the diagonal metric: k_nuts {fmt(td)}, {leap1} leapfrog steps, {per(td, leap1):.1f} ps per step and chain; "
            f"k_nuts_dense at diag(1 / dmm) {fmt(tn)}, {leap2} leapfrog steps, {per(tn, leap2):.1f} ps per step and chain; dense / diagonal {np.median(tn) / np.median(td):.3f}")
        # (b) each sampler under its own adapted metric
        rows = {}
        for name, res, st, kw in (("diagonal", diag, st_diag, dict(dmm=diag.dmm)), ("dense", dense, st_dense, dict(sigma=dense.inv_metric))):
            ts = []
            for r in range(a.repeats + 1):
                t, leap, dsum = launch(L, model, st, a.sample, res.eps, a.max_depth, ev, **kw)
                if r:
                    ts.append(t)
            ess, j, acc, ndiv = ess_run(model, st.astype(np.float64), res.kernel, a.sample)
            rows[name] = (np.median(ts), leap / (a.chains * a.sample), ess / np.median(ts))
            say(f"(b) {dtype} {name} after W = {a.warmup}: eps {res.eps:.4g}, mean depth {dsum / (a.chains * a.sample):.2f}, leapfrog steps per iteration {leap / (a.chains * a.sample):.2f}, "
                f"{a.sample} iterations {fmt(ts)}, mean accept {acc:.3f}, divergent {ndiv}, min ESS per chain set {ess:.0f} (coordinate {j}), min-ESS/s {ess / np.median(ts):.4g}")
        say(f"(b) {dtype} dense / diagonal: time {rows['dense'][0] / rows['diagonal'][0]:.3f}, leapfrog steps {rows['dense'][1] / rows['diagonal'][1]:.3f}, "
            f"min-ESS/s {rows['dense'][2] / rows['diagonal'][2]:.3f}")
        cor = dense.inv_metric / np.sqrt(np.outer(np.diag(dense.inv_metric), np.diag(dense.inv_metric)))
        say(f"(b) {dtype} adapted dense metric: sd {np.array2string(np.sqrt(np.diag(dense.inv_metric)), precision=4)}, condition number of its correlation matrix "
            f"{np.linalg.cond(cor):.1f}, largest |correlation| {np.max(np.abs(cor - np.eye(8))):.3f}")
        model.close()
    from logreg_amd import build as b
    rows = [r for r in b.kernel_resources() if "k_nuts_dense<" in r["name"]]
    if not rows:
        say("(c) the object files of the build are not here (logreg_amd/lib/obj): run this script where the library was built for the kernels' resources")
    for r in rows:  # (gfx950: one unified file of 512 registers per lane and SIMD; a 256-lane workgroup is one wave per SIMD)
        T, P = ("float", 4) if "<float" in r["name"] else ("double", 8), int(r["name"].split(",")[1])
        say(f"(c) {r['name'].split('(')[0].replace('void lr::', '')}: {r['vgprs']} VGPRs ({r['agprs']} of them in the accumulator half), {r['sgprs']} SGPRs, scratch {r['scratch']} B, "
            f"{min(8, 512 // max(r['vgprs'], 1))} wave(s) per SIMD by registers; dynamic LDS with 768 rows at max_depth 10: rows {768 * (P + (0 if T[1] == 4 else 2)) * T[1]} + checkpoints "
            f"{2 * 10 * ((P + 15) // 16) * 256 * T[1]} + matrices {2 * P * P * T[1]} B")
    return 0


if __name__ == "__main__":
    sys.exit(main())
