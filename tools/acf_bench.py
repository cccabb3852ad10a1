#!/usr/bin/env python3
"""Cost of the autocorrelation / Geyer-ESS accumulator (csrc/lr_acf.h), beside the host's way to the same number:
    python3 tools/acf_bench.py [--out profiles/r11_acf.txt] [--scale N]

1. Accumulate: C x p = 8 x n = 1000 kept draws of float32, C in {4096, 65536}, K in {63, 255}; the draws are on the device before the
   clock starts (as they are after sampling).  One call of 1000 steps, and the same draws in 20 calls of 50 (as mcmc's chunks arrive):
   HIP events, one warm run, then the median of at least 10.  The float64 FMA rate C p n (K + 1) / t is given as a fraction of the
   vector peak (CUs x 64 lanes x 2.4 GHz FMA/s); lr_acf_result is timed the same way.
2. The host's way (what the parent commit offers): `to_host()` of the block + `diagnostics.ess_pooled(max_chains=None)`, wall clock, in
   this process.  At 65 536 chains it is timed on the first 4096 chains and multiplied by 16 (said in the line).
3. The headline shape: 4096 chains of Pima HMC, thin 20, L = 50, 1000 kept draws in chunks of 50, K = 63.  Per chunk HIP events bracket the
   sampling launch and the fold; cost = sum of folds / sum of sampling.  REQUIREMENT: under 2 %.
4. Error / bound ratios of the test set: `python tests/test_gpu_acf.py --measure` (its FIGURE lines are appended when --ratios is given).
"""
import argparse
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

CLOCK = 2.4e9


def accumulate_shape(Cn, p, n, K, lines, host_chains):
    L = _lib.load()
    rng = np.random.default_rng(Cn + K)
    base = min(Cn, 4096)  # (beyond 4096 chains the same series again: the clock does not read them)
    xb = np.empty((n, base, p), dtype=np.float32)
    z = rng.standard_normal((base, p)).astype(np.float32)
    for t in range(n):  # AR(1), phi = 0.9
        z = np.float32(0.9) * z + np.float32(np.sqrt(1 - 0.81)) * rng.standard_normal((base, p)).astype(np.float32)
        xb[t] = 3.0 + 0.5 * z
    x = np.tile(xb, (1, Cn // base, 1)) if Cn > base else xb
    dx = la.DeviceArray.from_host(0, x)
    ac = la.Autocorr(Cn, p, "float32", max_lag=K)
    ac.update(dx.rows(0, 1))
    ev = Events(L, 0)
    peak = L.lr_device_cus(0) * 64 * CLOCK
    fmas = float(Cn) * p * n * (K + 1)

    t_one = repeats(ev.time, lambda: ac.update(dx), before=ac.reset)

    def chunks():
        for t0 in range(0, n, 50):
            ac.update(dx.rows(t0, min(t0 + 50, n)))
    t_chunks = repeats(ev.time, chunks, before=ac.reset)
    t_res = repeats(ev.time, ac.sums)
    res = ac.result()
    mo, mc, mr = float(np.median(t_one)), float(np.median(t_chunks)), float(np.median(t_res))
    line = (f"accumulate C={Cn} p={p} n={n} K={K} float32: one call {mo * 1e3:.3f} ms (min {t_one.min() * 1e3:.3f}, max {t_one.max() * 1e3:.3f}, n={len(t_one)}) = "
            f"{fmas / mo:.3e} FMA/s = {fmas / mo / peak:.3f} of the fp64 vector peak | 20 calls of 50: {mc * 1e3:.3f} ms (min {t_chunks.min() * 1e3:.3f}, "
            f"max {t_chunks.max() * 1e3:.3f}) = {fmas / mc / peak:.3f} of peak | lr_acf_result {mr * 1e3:.3f} ms | state {Cn * p * (3 * K + 3) * 8 / 2**20:.0f} MiB")
    print(line, flush=True)
    lines.append(line)
    if host_chains:
        t0 = time.perf_counter()
        host = dx.to_host()
        t_copy = time.perf_counter() - t0
        sub = host[:, :host_chains].astype(np.float64)
        t0 = time.perf_counter()
        ess = la.ess_pooled(sub, max_chains=None)
        t_ess = (time.perf_counter() - t0) * (Cn / host_chains)
        mine = res["ess_chain"][:host_chains].sum(axis=0)
        capped = float(res["capped"].sum())
        line = (f"host way   C={Cn} p={p} n={n}: to_host {t_copy * 1e3:.1f} ms + ess_pooled(max_chains=None) {t_ess:.2f} s"
                f"{'' if host_chains == Cn else f' (timed on {host_chains} chains, x {Cn // host_chains})'} = {(t_copy + t_ess) / (mo + mr):.0f} x accumulate + result; "
                f"largest relative difference of the pooled ESS over those chains {float(np.max(np.abs(mine - ess) / ess)):.2e} ({capped:.0f} capped series at K={K})")
        print(line, flush=True)
        lines.append(line)
    ac.free()
    dx.free()
    return fmas / mo / peak


def headline(lines, chains, iters, thin, l, K, chunk):
    X, y = la.load_pima()
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    init = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
    model = la.LogReg(X, y, pscale, dtype="float32")
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=l, dmm=1 / pre)
    cs = la.ChainSet(kern, np.tile(init, (chains, 1)), seed=1)
    ac = la.Autocorr(chains, 8, "float32", max_lag=K)
    ev = Events(model._L, 0, cs.stream)
    out = cs.advance(chunk, thin)  # warm: clocks, the accumulator's state
    ac.update(out, stream=cs.stream)
    cs.sync()
    ac.reset()
    t_sample, t_fold = [], []
    hold = {}
    for _ in range(iters // chunk):
        t_sample.append(ev.time(lambda: hold.update(out=cs.advance(chunk, thin, out=out))))
        t_fold.append(ev.time(lambda: ac.update(out, stream=cs.stream)))
    cs.sync()
    res = ac.result()
    ts, tf = float(np.sum(t_sample)), float(np.sum(t_fold))
    kept = (iters // chunk) * chunk
    line = (f"headline {chains} chains x {kept} kept draws, thin {thin}, L = {l}, K = {K}, chunks of {chunk}: sampling {ts * 1e3:.1f} ms, folding {tf * 1e3:.3f} ms "
            f"= {100 * tf / ts:.3f} % of the sampling time (requirement: < 2 %) | Geyer ESS per coordinate (sum over chains) {np.round(res['ess']).astype(np.int64).tolist()}, "
            f"ESS/s {np.min(res['ess']) / ts:.3e} (smallest coordinate), capped series {int(res['capped'].sum())}")
    print(line, flush=True)
    lines.append(line)
    ac.free()
    out.free()
    model.close()
    return tf / ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the chain counts (a quick look)")
    ap.add_argument("--ratios", action="store_true", help="append the FIGURE lines of tests/test_gpu_acf.py --measure (a child process)")
    a = ap.parse_args()
    lines = [_lib.device_info(0)]
    print(lines[0], flush=True)
    for Cn in (4096 // a.scale, 65536 // a.scale):
        for K in (63, 255):
            accumulate_shape(Cn, 8, 1000, K, lines, host_chains=min(Cn, 4096 // a.scale) if K == 63 else 0)
    share = headline(lines, 4096 // a.scale, 1000, 20, 50, 63, 50)
    if a.ratios:
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "test_gpu_acf.py"), "--measure"], capture_output=True, text=True, timeout=900)
        fig = [ln for ln in r.stdout.split("\n") if ln.startswith("FIGURE")]
        if r.returncode != 0 or not fig:
            fig = [f"tests/test_gpu_acf.py --measure failed (exit {r.returncode}): {r.stdout[-400:]} {r.stderr[-400:]}"]
        for ln in fig:
            print(ln, flush=True)
        lines.extend(fig)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if share < 0.02 else 1


if __name__ == "__main__":
    sys.exit(main())
