#!/usr/bin/env python3
"""Times of the two stages of PSIS-LOO (csrc/lr_loo.h) beside torch on the same resident draws:
    python3 tools/loo_bench.py [--out FILE]         (its lines are section 2 of profiles/r14_loo.txt; needs the GPU)
    python3 tools/loo_bench.py --resources          (registers and LDS of the kernels from the code objects; needs the object files, no GPU)

Shapes (draws S, rows n, width p): (4096 x 64, 200 = Pima, 8) and (4096, 100 000, 8), float32 and float64.  The draws are on the device
before the clock starts (as they are after sampling).  Per shape and stage: one warm call, then 10 calls timed one by one with HIP
events; the median is reported with the extremes.
    fill   PsisLoo.update of the whole block (k_loo_fill: the [n][S] matrix through LDS tiles)
    psis   PsisLoo.table (k_psis over every row, and the copy of the [5, n] table)

Yardstick: what a user can do today without the accumulator -- torch on the same draws buffer (viewed through
__cuda_array_interface__, no copy): fill = logsigmoid(B @ Xs^T) as one [S, n] matrix; psis = a per-row topk of the M largest importance
ratios and a sort of them (the order statistics PSIS needs; the Pareto fit and the sums are NOT in the yardstick, which flatters it).
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
from logreg_amd.loo import tail_length  # noqa: E402

RUNS = 10


def resources():
    from logreg_amd import build
    rows = [r for r in build.kernel_resources() if "k_psis" in r["name"] or "k_loo_" in r["name"]]
    return [f"{r['name'].split('(')[0]}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, {r['lds']} bytes of LDS, {r['scratch']} bytes of scratch" for r in rows]


def hip_timer(L, device):
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.lr_event_create(device, C.byref(a)))
    _lib.check(L.lr_event_create(device, C.byref(b)))

    def time(fn):
        ms = C.c_float()
        _lib.check(L.lr_event_record(device, a, None))
        fn()
        _lib.check(L.lr_event_record(device, b, None))
        _lib.check(L.lr_stream_sync(device, None))
        _lib.check(L.lr_event_elapsed_ms(device, a, b, C.byref(ms)))
        return ms.value * 1e-3
    return time


def torch_timer(torch):
    def time(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    return time


def median_of(timer, fn):
    timer(fn)  # warm
    t = np.array([timer(fn) for _ in range(RUNS)])
    return float(np.median(t)), float(t.min()), float(t.max())


def shape(name, X, y, pscale, S, dtype, center, spread, lines):
    import torch
    model = la.LogReg(X, y, pscale, dtype=dtype)
    n, p = X.shape
    rng = np.random.default_rng(1)
    B = (center[None, :] + spread * rng.standard_normal((S, p))).astype(model.np_dtype)
    dB = la.DeviceArray.from_host(model.device, B)
    acc = la.PsisLoo(model, S)
    ht = hip_timer(model._L, model.device)

    def fill():
        acc.reset()
        acc.update(dB)
    f = median_of(ht, fill)
    q = median_of(ht, acc.table)
    res = acc.result()

    dev = torch.device("cuda", model.device)
    Bt = torch.as_tensor(dB, device=dev)
    assert Bt.data_ptr() == dB.ptr  # the same buffer
    Xs = torch.as_tensor(((2 * y - 1)[:, None] * X).astype(model.np_dtype), device=dev)
    M = tail_length(S)
    tt = torch_timer(torch)
    keep = {}

    def tfill():
        keep["ll"] = torch.nn.functional.logsigmoid(Bt @ Xs.T)

    def tpsis():
        keep["tail"] = torch.sort(torch.topk(-keep["ll"], M, dim=0).values, dim=0).values
    tf = median_of(tt, tfill)
    tq = median_of(tt, tpsis)
    agree = float(np.max(np.abs(keep["ll"][:4096].cpu().numpy().astype(np.float64) - acc.loglik()[:4096].astype(np.float64)))) if S * n <= 1 << 28 else float("nan")
    line = (f"{name} {dtype}: S={S} n={n} p={p} M={M} | fill: fused {f[0] * 1e3:.3f} ms (min {f[1] * 1e3:.3f}, max {f[2] * 1e3:.3f}), torch {tf[0] * 1e3:.3f} ms "
            f"(min {tf[1] * 1e3:.3f}, max {tf[2] * 1e3:.3f}), torch / fused = {tf[0] / f[0]:.2f} | psis: fused {q[0] * 1e3:.3f} ms (min {q[1] * 1e3:.3f}, max {q[2] * 1e3:.3f}), "
            f"torch topk + sort {tq[0] * 1e3:.3f} ms (min {tq[1] * 1e3:.3f}, max {tq[2] * 1e3:.3f}), torch / fused = {tq[0] / q[0]:.2f} | both: torch / fused = "
            f"{(tf[0] + tq[0]) / (f[0] + q[0]):.2f} | elpd_loo {res['elpd_loo']:.4f}, {res['n_khat_over_0_7']} k-hat over 0.7 | max |fused - torch| on the matrix {agree:.2e}")
    print(line, flush=True)
    lines.append(line)
    acc.close()
    dB.free()
    model.close()
    return tf[0] / f[0], tq[0] / q[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the draw and row counts (a quick look)")
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers and LDS from the code objects and exit")
    a = ap.parse_args()
    if a.resources:
        print("\n".join(resources()))
        return 0
    import torch
    torch.cuda.init()  # the yardstick needs its device: fail here, before any work, if torch finds none
    lines = [_lib.device_info(0), f"median of {RUNS} runs after a warm run, HIP events"]
    print(lines[0], flush=True)
    X, y = la.load_pima()
    mp = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
    sd = np.array([1.71, 0.0655, 0.0068, 0.0184, 0.0226, 0.0429, 0.547, 0.0225]) * 0.3
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    Xt, yt, bt = la.synthetic_logreg(100000 // a.scale, 8)
    ratios = []
    for dtype in ("float32", "float64"):
        ratios += shape("pima", X, y, ps, 4096 * 64 // a.scale, dtype, mp, sd, lines)
        ratios += shape("tall", Xt, yt, np.ones(8), 4096, dtype, bt, 0.02, lines)
    verdict = f"slowest torch / fused ratio over the shapes and stages: {min(ratios):.2f}" + ("" if min(ratios) >= 1 else "  -- the fused path LOSES to the yardstick there")
    print(verdict)
    lines.append(verdict)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
