#!/usr/bin/env python3
"""Cost of the marginals accumulator (csrc/lr_marginals.h):
    python3 tools/marginals_bench.py [--out profiles/r12_marginals.txt] [--scale N] [--ratios]

1. One lr_marg_accumulate of a block [64, C, 8] that is already on the device (as it is after sampling): float32 and float64, C in {4096,
   65536}, bins in {64, 256, 1024}; HIP events, one warm run, then the median of 10 (min and max beside it).  The draws are normal about
   the grid's centre with the grid at -+ 8 sd.  Beside each: the bytes of the block over the time, as a fraction of what a
   device-to-device copy of the same block reaches (the bandwidth floor: a copy reads and writes, the accumulator only reads, so 2.0
   would be the floor itself), and lr_acf_accumulate at K = 63 on the same block.
2. The contention case: the same shapes with a CONSTANT block (every lane of a workgroup that shares a coordinate on one LDS counter).
3. p = 128 at C = 4096: bins 64 (the flat lane map) and 256, 1024 (tables beyond the LDS budget: the tiled lane map).
4. lr_marg_result, timed the same way.
5. The headline run (4096 chains of Pima HMC, thin 20, L = 50, 1000 kept draws, summary_only=True): wall time with and without marginals=.
6. With --ratios: the FIGURE lines of `python tests/test_gpu_marginals.py --measure` (a child process).
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


def fmt(t):
    return f"{np.median(t) * 1e3:.3f} ms (min {t.min() * 1e3:.3f}, max {t.max() * 1e3:.3f})"


def block_of(Cn, p, k, dtype, constant):
    if constant:
        return np.full((k, Cn, p), 0.25, dtype=dtype)
    rng = np.random.default_rng(Cn + p)
    base = min(Cn, 4096)  # (beyond 4096 chains the same draws again: the clock does not read them)
    xb = rng.standard_normal((k, base, p)).astype(dtype)
    return np.tile(xb, (1, Cn // base, 1)) if Cn > base else xb


def shape(Cn, p, k, dtype, constant, bins_list, lines, with_floor):
    L = _lib.load()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    x = block_of(Cn, p, k, dtype, constant)
    dx = la.DeviceArray.from_host(0, x)
    ev = Events(L, 0)
    tag = f"C={Cn} p={p} k={k} {dtype}{' CONSTANT block' if constant else ''}"
    floor = ""
    t_copy = None
    if with_floor:
        dy = la.DeviceArray.from_host(0, x)
        t_copy = repeats(ev.time, lambda: hip.hipMemcpyAsync(dy.ptr, dx.ptr, x.nbytes, 3, None))  # 3: device to device
        dy.free()
        ac = la.Autocorr(Cn, p, dtype, max_lag=63)
        ac.update(dx.rows(0, 1))
        t_acf = repeats(ev.time, lambda: ac.update(dx), before=ac.reset)
        ac.free()
        line = f"floor      {tag}: device-to-device copy of the block ({x.nbytes / 2**20:.1f} MiB) {fmt(t_copy)} = {x.nbytes / np.median(t_copy) / 1e9:.0f} GB/s copied | lr_acf_accumulate K=63 {fmt(t_acf)}"
        print(line, flush=True)
        lines.append(line)
    for bins in bins_list:
        mg = la.Marginals(Cn, p, dtype, -8.0 * np.ones(p), 8.0 * np.ones(p), bins=bins)
        mg.update(dx.rows(0, 1))
        t = repeats(ev.time, lambda: mg.update(dx), before=mg.reset)
        t_res = repeats(ev.time, mg.counts_table)
        counts, _ = mg.counts_table()
        assert int(counts.sum()) == k * Cn * p
        if t_copy is not None:
            floor = f" = {np.median(t) / np.median(t_copy):.2f} x the copy"
        line = (f"accumulate {tag} bins={bins}: {fmt(t)} = {x.nbytes / np.median(t) / 1e9:.0f} GB/s read, {k * Cn * p / np.median(t) / 1e9:.2f} G draws/s{floor} | "
                f"lr_marg_result {np.median(t_res) * 1e3:.3f} ms")
        print(line, flush=True)
        lines.append(line)
        mg.free()
    dx.free()


def headline(lines, chains, iters, thin, l):
    X, y = la.load_pima()
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    beta, info = la.find_map(la.LogReg(X, y, pscale, dtype="float64"))
    model = la.LogReg(X, y, pscale, dtype="float32")
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=l, dmm=1 / pre)
    init = np.tile(beta, (chains, 1))
    lo, hi = la.marginal_grid(beta, info["sd"])
    kw = dict(thin=thin, iters=iters, verb=False, summary_only=True, seed=2)
    la.mcmc(init, kern, thin=thin, iters=50, verb=False, summary_only=True, seed=1)  # warm: clocks, code objects
    walls = {}
    for label in ("without", "with", "without again", "with again"):
        mg = la.Marginals(chains, 8, "float32", lo, hi) if label.split()[0] == "with" else None
        if mg is not None:
            mg.update(np.zeros((1, chains, 8), dtype=np.float32)).reset()  # (the state is allocated outside the clock)
        t0 = time.perf_counter()
        res = la.mcmc(init, kern, marginals=mg, **kw)
        walls[label] = time.perf_counter() - t0
        if mg is not None:
            r = res["marginals"]
            mg.free()
    line = (f"headline {chains} chains x {iters} kept draws, thin {thin}, L = {l}, summary_only=True, wall: " + ", ".join(f"{k} marginals= {v:.3f} s" for k, v in walls.items())
            + f" | skewness {np.round(r['skewness'], 3).tolist()} kurtosis {np.round(r['kurtosis'], 3).tolist()} outside the grid {int(r['underflow'].sum() + r['overflow'].sum())}")
    print(line, flush=True)
    lines.append(line)
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the chain counts (a quick look)")
    ap.add_argument("--ratios", action="store_true", help="append the FIGURE lines of tests/test_gpu_marginals.py --measure (a child process)")
    a = ap.parse_args()
    lines = [_lib.device_info(0)]
    print(lines[0], flush=True)
    for dtype in ("float32", "float64"):
        for Cn in (4096 // a.scale, 65536 // a.scale):
            shape(Cn, 8, 64, dtype, False, (64, 256, 1024), lines, with_floor=True)
            shape(Cn, 8, 64, dtype, True, (64, 256, 1024), lines, with_floor=False)
        shape(4096 // a.scale, 128, 64, dtype, False, (64, 256, 1024), lines, with_floor=True)
    headline(lines, 4096 // a.scale, 1000, 20, 50)
    if a.ratios:
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "test_gpu_marginals.py"), "--measure"], capture_output=True, text=True, timeout=900)
        fig = [ln for ln in r.stdout.split("\n") if ln.startswith("FIGURE")]
        if r.returncode != 0 or not fig:
            fig = [f"tests/test_gpu_marginals.py --measure failed (exit {r.returncode}): {r.stdout[-400:]} {r.stderr[-400:]}"]
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
