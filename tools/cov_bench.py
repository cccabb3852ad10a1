#!/usr/bin/env python3
"""Cost of the covariance accumulator (csrc/lr_cov.h):
    python3 tools/cov_bench.py [--out profiles/r16_cov.txt] [--scale N] [--ratios]

1. One lr_cov_accumulate of a block [64, C, p] that is already on the device (as it is after sampling): 4096 x 8 float32, 65 536 x 8 and
   4096 x 128 in float32 and float64; HIP events, one warm run, then the median of 10 (min and max beside it).  Beside each: the
   device-to-device copy of the same block (the bytes bound: a copy reads and writes, the accumulator only reads), lr_marg_accumulate at
   bins 256 on the same block, and the fma bound: N P (P + 1) / 2 float64 fma over the fp64 vector peak of DESIGN.md (78.6 TF: 256 CUs x 4 SIMDs x
   16 lanes x 2.4 GHz = 3.93e13 fma/s).
2. lr_cov_result (all four tables), timed the same way.
3. The headline run (4096 chains of Pima HMC, thin 20, L = 50, 1000 kept draws, summary_only=True): wall time with and without covariance=.
4. With --ratios: the FIGURE lines of `python tests/test_gpu_cov.py --measure` (a child process).
Every number is recorded; none is a requirement.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402
from bench_util import Events, repeats  # noqa: E402

FMA_F64_PEAK = 256 * 4 * 16 * 2.4e9  # float64 vector fma per second (78.6 TF)


def fmt(t):
    return f"{np.median(t) * 1e3:.3f} ms (min {t.min() * 1e3:.3f}, max {t.max() * 1e3:.3f})"


def shape(Cn, p, k, dtype, lines):
    L = _lib.load()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rng = np.random.default_rng(Cn + p)
    base = min(Cn, 4096)  # (beyond 4096 chains the same draws again: the clock does not read them)
    xb = rng.standard_normal((k, base, p)).astype(dtype)
    x = np.tile(xb, (1, Cn // base, 1)) if Cn > base else xb
    dx = la.DeviceArray.from_host(0, x)
    ev = Events(L, 0)
    tag = f"C={Cn} p={p} k={k} {dtype} ({x.nbytes / 2**20:.0f} MiB)"
    dy = la.DeviceArray.from_host(0, x)
    t_copy = repeats(ev.time, lambda: hip.hipMemcpyAsync(dy.ptr, dx.ptr, x.nbytes, 3, None))  # 3: device to device
    dy.free()
    mg = la.Marginals(Cn, p, dtype, -8.0 * np.ones(p), 8.0 * np.ones(p), bins=256)
    mg.update(dx.rows(0, 1))
    t_marg = repeats(ev.time, lambda: mg.update(dx), before=mg.reset)
    mg.free()
    acc = la.Covariance(Cn, p, dtype, np.zeros(p), np.ones(p))
    acc.update(dx.rows(0, 1))
    t = repeats(ev.time, lambda: acc.update(dx), before=acc.reset)
    t_res = repeats(ev.time, acc.tables)
    M = acc.tables()[0]
    assert np.all(np.isfinite(M)) and np.all(np.diag(M) > 0)
    acc.free()
    P = 4 if p <= 4 else 1 << int(np.ceil(np.log2(p)))
    fma = k * Cn * P * (P + 1) / 2
    t_fma, med = fma / FMA_F64_PEAK, np.median(t)
    bound = "bytes" if np.median(t_copy) > t_fma else "fma"
    line = (f"accumulate {tag}: {fmt(t)} = {x.nbytes / med / 1e9:.0f} GB/s read, {k * Cn / med / 1e9:.3f} G draws/s, {fma / med / 1e12:.2f} T fma/s | copy {fmt(t_copy)} "
            f"({med / np.median(t_copy):.2f} x the copy) | fma bound {t_fma * 1e3:.3f} ms ({med / t_fma:.1f} x) | nearer bound: {bound} | "
            f"lr_marg_accumulate bins=256 {fmt(t_marg)} | lr_cov_result {fmt(t_res)}")
    print(line, flush=True)
    lines.append(line)
    dx.free()


def headline(lines, chains, iters, thin, l):
    X, y = la.load_pima()
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    beta, info = la.find_map(la.LogReg(X, y, pscale, dtype="float64"))
    model = la.LogReg(X, y, pscale, dtype="float32")
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=l, dmm=1 / pre)
    init = np.tile(beta, (chains, 1))
    center, scale = la.covariance_scaling(beta, info["sd"])
    kw = dict(thin=thin, iters=iters, verb=False, summary_only=True, seed=2)
    la.mcmc(init, kern, thin=thin, iters=50, verb=False, summary_only=True, seed=1)  # warm: clocks, code objects
    walls = {}
    for label in ("without", "with", "without again", "with again"):
        acc = la.Covariance(chains, 8, "float32", center, scale) if label.split()[0] == "with" else None
        if acc is not None:
            acc.update(np.zeros((1, chains, 8), dtype=np.float32)).reset()  # (the state is allocated outside the clock)
        t0 = time.perf_counter()
        res = la.mcmc(init, kern, covariance=acc, **kw)
        walls[label] = time.perf_counter() - t0
        if acc is not None:
            r = res["covariance"]
            acc.free()
    off = r["cor"][~np.eye(8, dtype=bool)]
    line = (f"headline {chains} chains x {iters} kept draws, thin {thin}, L = {l}, summary_only=True, wall: " + ", ".join(f"{k} covariance= {v:.3f} s" for k, v in walls.items())
            + f" | cor off the diagonal {off.min():.3f} .. {off.max():.3f}, rhat_mv {r['rhat_mv']:.5f}, max rhat {np.max(r['rhat']):.5f}")
    print(line, flush=True)
    lines.append(line)
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the chain counts (a quick look)")
    ap.add_argument("--ratios", action="store_true", help="append the FIGURE lines of tests/test_gpu_cov.py --measure (a child process)")
    a = ap.parse_args()
    lines = [_lib.device_info(0)]
    print(lines[0], flush=True)
    shape(4096 // a.scale, 8, 64, "float32", lines)
    for dtype in ("float32", "float64"):
        shape(65536 // a.scale, 8, 64, dtype, lines)
    for dtype in ("float32", "float64"):
        shape(4096 // a.scale, 128, 64, dtype, lines)
    headline(lines, 4096 // a.scale, 1000, 20, 50)
    if a.ratios:
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "test_gpu_cov.py"), "--measure"], capture_output=True, text=True, timeout=900)
        fig = [ln for ln in r.stdout.split("\n") if ln.startswith("FIGURE")]
        if r.returncode != 0 or not fig:
            fig = [f"tests/test_gpu_cov.py --measure failed (exit {r.returncode}): {r.stdout[-400:]} {r.stderr[-400:]}"]
        for ln in fig:
            print(ln, flush=True)
        lines.extend(fig)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
