#!/usr/bin/env python3
"""The Polya-Gamma Gibbs kernel on Pima, measured (needs an MI355X): sweeps/s, min-ESS/s from the Autocorr accumulator beside the
reference's HMC setting (eps 1e-3, L 50, dmm 1 / pre, thin 20) at the same chain count in the same process, the counters' ratios, and
registers / LDS / occupancy per instantiation.  Writes the report to the path given; profiles/r21_pg.txt holds one such report.

    python tools/pg_bench.py [--chains 4096,65536] [--kept 64] [--out pg_bench.txt]

Times are host clocks around launches that end in a stream synchronise, best of three after a warm-up launch of the same shape.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import logreg_amd as la  # noqa: E402
from logreg_amd import build  # noqa: E402


def timed(cs, iters, thin, repeats=3, window=0.3):
    """-> (seconds, iters): best of `repeats` launches of a length that a pilot launch of `iters` puts at `window` seconds or more"""
    cs.advance(1, thin, keep=False)
    cs.sync()
    t0 = time.perf_counter()
    cs.advance(iters, thin, keep=False)
    cs.sync()
    pilot = time.perf_counter() - t0
    iters = int(max(iters, np.ceil(iters * window / max(pilot, 1e-6))))
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        cs.advance(iters, thin, keep=False)
        cs.sync()
        best = min(best, time.perf_counter() - t0)
    return best, iters


def ess_per_kept(kernel, start, kept, thin, burn, dtype, seed):
    """Geyer ESS per kept draw and coordinate (pooled over chains) from the on-device accumulator"""
    C, p = start.shape
    cs = la.ChainSet(kernel, start, seed=seed)
    cs.advance(1, burn, keep=False)
    ac = la.Autocorr(C, p, dtype, max_lag=31)
    done = 0
    while done < kept:
        k = min(16, kept - done)
        out = cs.advance(k, thin)
        ac.update(out, stream=cs.stream)
        cs.sync()
        out.free()
        done += k
    return ac.result()["ess"] / (C * kept), cs


def resources():
    """registers, LDS and occupancy of the eight instantiations, from the AMDGPU metadata of the built objects (where they exist)"""
    rows = [r for r in build.kernel_resources() if "k_pg<" in r["name"]]
    if not rows:
        return ["registers and LDS per instantiation: no object files here (python tools/pg_bench.py --resources where the library was built)"]
    lines = ["registers, LDS and occupancy per instantiation (AMDGPU metadata of the built objects; occupancy = waves per SIMD that 512 registers",
             "allow; the LDS is all dynamic: rows + 16 n elements of omega staging -- Pima float32 6400 + 12 800 bytes, float64 16 000 + 25 600):"]
    for r in rows:
        regs = r["vgprs"] + r["agprs"]
        lines.append(f"    {r['name'].split('(')[0]:32s} vgprs {r['vgprs']:3d} agprs {r['agprs']:3d} sgprs {r['sgprs']:3d} scratch {r['scratch']} static LDS {r['lds']} "
                     f"-> {max(1, 512 // max(regs, 1))} waves per SIMD")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="4096,65536")
    ap.add_argument("--kept", type=int, default=64)
    ap.add_argument("--out", default="pg_bench.txt")
    ap.add_argument("--resources", action="store_true", help="only the register / LDS table of the built objects (needs no GPU)")
    a = ap.parse_args()
    if a.resources:
        print("\n".join(resources()))
        return
    la._lib.require_gpu()
    X, y = la.load_pima()
    n, p = X.shape
    pscale = np.array([10., 1., 1., 1., 1., 1., 1., 1.])
    pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
    beta, _ = la.find_map(la.LogReg(X, y, pscale, dtype="float64"), np.zeros(p))
    lines = [f"device: {la._lib.device_info(0)}", f"Pima n = {n}, p = {p}; chains start at the MAP; PG: 50 sweeps discarded, {a.kept} kept at thin 1; "
             f"HMC (the reference's fit-np-hmc.py setting: eps 1e-3, L 50, dmm 1 / pre): 20 kept draws of thin 20 discarded, {a.kept} kept at thin 20", ""]
    for C in [int(c) for c in a.chains.split(",")]:
        start = np.tile(beta, (C, 1))
        for dtype in ("float32", "float64"):
            m = la.LogReg(X, y, pscale, dtype=dtype)
            pg = la.pgKernel(m.lpost)
            ess, cs = ess_per_kept(pg, start, a.kept, 1, 50, dtype, 11)
            info = cs.pg_info()
            t, k = timed(cs, 50, 1)
            sweeps_s = C * k / t
            lines.append(f"PG  {dtype} {C:6d} chains: {t * 1e3:9.2f} ms per {k} sweeps, {sweeps_s:.4g} sweeps/s, ESS per kept sweep {ess.min():.3f} .. {ess.max():.3f}, "
                         f"min-ESS/s {ess.min() * sweeps_s:.4g}; proposals per draw {info['proposals_per_draw'].mean():.5f}, series terms per draw "
                         f"{info['series_terms_per_draw'].mean():.5f}, skipped {int(info['skipped'].sum())}; plan {cs.plan()}")
            hk = la.hmcKernel(m.lpost, m.glp, eps=1e-3, l=50, dmm=1.0 / pre)
            ess_h, cs_h = ess_per_kept(hk, start, a.kept, 20, 400, dtype, 11)
            t_h, k_h = timed(cs_h, 5, 20)
            kept_s = C * k_h / t_h
            lines.append(f"HMC {dtype} {C:6d} chains: {t_h * 1e3:9.2f} ms per {k_h} kept draws of thin 20, {kept_s * 20:.4g} iterations/s, ESS per kept draw "
                         f"{ess_h.min():.3f} .. {ess_h.max():.3f}, min-ESS/s {ess_h.min() * kept_s:.4g}; plan {cs_h.plan()}")
            lines.append(f"    min-ESS/s, PG over HMC: {ess.min() * sweeps_s / (ess_h.min() * kept_s):.2f}")
            m.close()
        lines.append("")
    lines += resources()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
