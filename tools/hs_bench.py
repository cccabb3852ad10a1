#!/usr/bin/env python3
"""The horseshoe Polya-Gamma kernel beside the Polya-Gamma kernel, measured (needs an MI355X): sweeps/s of k_hs and k_pg on the same model
and chain counts (Pima at 4096 and 65 536 chains; a sparse n = 150, p = 24 design), their ratio -- the cost of the hyper-step -- and
the registers of every instantiation in both builds.  Writes the report to the path given; profiles/r30_hs.txt holds one such report.

    python tools/hs_bench.py [--chains 4096,65536] [--out hs_bench.txt]
    python tools/hs_bench.py --resources        (the register table alone: needs the built objects, no GPU)

Times are host clocks around launches that end in a stream synchronise, best of three after a warm-up launch of the same shape.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import logreg_amd as la  # noqa: E402
from logreg_amd import build  # noqa: E402
from pg_bench import timed  # noqa: E402


def resources():
    """registers of the sixteen instantiations in both builds, from the AMDGPU metadata of the built objects (where they exist)"""
    lines = []
    for alt in (False, True):
        rows = [r for r in build.kernel_resources(alt=alt) if "k_pg<" in r["name"] or "k_hs<" in r["name"]]
        if not rows:
            lines.append(("second build" if alt else "production build") + ": no object files here (python tools/hs_bench.py --resources where the library was built)")
            continue
        lines.append(("second build (lib_alt)" if alt else "production build") + ": registers per instantiation (512 per lane at one wave per SIMD; the LDS is k_pg's, all dynamic)")
        for r in sorted(rows, key=lambda r: (r["unit"], r["name"])):
            lines.append(f"    {r['name'].split('(')[0]:32s} vgprs {r['vgprs']:3d} agprs {r['agprs']:3d} sgprs {r['sgprs']:3d} scratch {r['scratch']} static LDS {r['lds']}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="4096,65536")
    ap.add_argument("--out", default="hs_bench.txt")
    ap.add_argument("--resources", action="store_true", help="only the register table of the built objects (needs no GPU)")
    a = ap.parse_args()
    if a.resources:
        print("\n".join(resources()))
        return
    la._lib.require_gpu()
    Xp, yp = la.load_pima()
    rng = np.random.default_rng(1)
    Xs = rng.standard_normal((150, 24))
    Xs[:, 0] = 1.0
    truth = np.zeros(24)
    truth[[1, 5, 9, 17]] = [2.0, -1.5, 1.5, -2.0]
    ys = (rng.random(150) < 1.0 / (1.0 + np.exp(-Xs @ truth))).astype(np.float64)
    shapes = [("Pima n = 200, p = 8", Xp, yp, np.array([10., 1., 1., 1., 1., 1., 1., 1.])), ("sparse n = 150, p = 24", Xs, ys, np.full(24, 5.0))]
    lines = [f"device: {la._lib.device_info(0)}", "k_hs beside k_pg: chains start at 0, 50 sweeps discarded, then launches of 50 sweeps or more (0.3 s at least), best of three", ""]
    for name, X, y, ps in shapes:
        n, p = X.shape
        tau0 = 4 / (p - 1 - 4) / np.sqrt(n) if p > 8 else 1.0
        for C in [int(c) for c in a.chains.split(",")]:
            for dtype in ("float32", "float64"):
                m = la.LogReg(X, y, ps, dtype=dtype)
                rate = {}
                for kind, k in (("pg", la.pgKernel(m.lpost)), ("hs", la.hsKernel(m.lpost, global_scale=tau0))):
                    cs = la.ChainSet(k, np.zeros((C, p)), seed=11)
                    cs.advance(1, 50, keep=False)
                    t, it = timed(cs, 50, 1)
                    rate[kind] = C * it / t
                    info = cs.pg_info()
                    lines.append(f"{name}, {dtype} {C:6d} chains, k_{kind}: {t * 1e3:9.2f} ms per {it} sweeps, {rate[kind]:.4g} sweeps/s, skipped {int(info['skipped'].sum())}"
                                 + (f", clamped {int(info['clamped'].sum())}" if kind == "hs" else ""))
                lines.append(f"    sweeps/s, k_hs over k_pg: {rate['hs'] / rate['pg']:.3f}")
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
