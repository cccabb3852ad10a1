#!/usr/bin/env python3
"""Throughput of the posterior-predictive accumulator (csrc/lr_predict.h) beside the same table computed with torch on the same device:
    python3 tools/predict_bench.py [--out FILE]      (its lines are section 2 of profiles/r9_predict.txt)

Shapes (draws S, prediction rows r, width p):
    S = 4096 x 1000, r = 200 (Pima's own rows), p = 8, float32 and float64
    S = 1024 x 200,  r = 4096, p = 128, float32
    S = 1024 x 50,   r = n = 100 000 (the model's own rows), p = 8, float32
The draws are on the device before the clock starts (as they are after sampling).  Each shape: one warm call, then repeats timed one by
one with HIP events until at least 0.5 s of work has been timed (at least 5 repeats).

Yardstick: what a user can do today without the accumulator -- torch on the same draws buffer (viewed through
__cuda_array_interface__, no copy): eta = B @ X.T, sigmoid, logsigmoid, and the five sums, chunked over the draws so that a [chunk, r]
matrix has at most 2^26 entries, sums accumulated in float64.  Same quantities, same buffers, same device.

Floor: the vector-issue time of the kernel's own hot loop -- its instruction mix per (draw, row) pair, counted in the ISA (DESIGN.md
"Prediction"), priced at MI355X issue costs with several waves per SIMD (float32 VALU 2 cycles, transcendental 8, float64 VALU 4.5,
v_rcp_f64 18: profiles/r3_trans_rate.txt, profiles/r6_f64_ops_rate.txt), 1024 SIMDs at 2.4 GHz.  "share" = floor / measured time: how
much of the time the binding resource (VALU + transcendental issue) explains."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402
from bench_util import Events, repeats_until as repeats  # noqa: E402

# hot-loop instruction mix per pair: (float32 VALU, transcendental, float64 VALU, v_rcp_f64), by (dtype, padded width) -- DESIGN.md "Prediction"
MIX = {("float32", 8): (17.2, 3, 10, 0), ("float64", 8): (16.8, 0, 72, 2), ("float32", 128): (140.6, 3, 10.1, 0)}
COST = (2.0, 8.0, 4.5, 18.0)
SIMDS, CLOCK = 1024, 2.4e9


def floor_seconds(dtype, P, pairs):
    cyc = sum(n * c for n, c in zip(MIX[(dtype, P)], COST))
    return pairs / 64.0 * cyc / (SIMDS * CLOCK)


def torch_table(torch, Bt, Xt, sgn, chunk):
    """The same five rows with torch (float64 accumulation of per-chunk sums; pivots: none -- plain sums and sums of squares)."""
    S = Bt.shape[0]
    r = Xt.shape[0]
    acc = torch.zeros((5, r), dtype=torch.float64, device=Bt.device)
    for a in range(0, S, chunk):
        eta = Bt[a:a + chunk] @ Xt.T
        pi = torch.sigmoid(eta)
        acc[0] += pi.sum(0, dtype=torch.float64)
        acc[1] += (pi * pi).sum(0, dtype=torch.float64)
        t = eta * sgn
        acc[2] += torch.sigmoid(t).sum(0, dtype=torch.float64)
        ls = torch.nn.functional.logsigmoid(t)
        acc[3] += ls.sum(0, dtype=torch.float64)
        acc[4] += (ls * ls).sum(0, dtype=torch.float64)
    out = torch.empty_like(acc)
    out[0] = acc[0] / S
    out[1] = acc[1] - acc[0] * acc[0] / S
    out[2] = acc[2] / S
    out[3] = acc[3] / S
    out[4] = acc[4] - acc[3] * acc[3] / S
    return out


def shape(name, X, y, pscale, Xnew, ynew, S, dtype, center, spread, lines):
    import torch
    model = la.LogReg(X, y, pscale, dtype=dtype)
    rng = np.random.default_rng(1)
    p = X.shape[1]
    B = (center[None, :] + spread * rng.standard_normal((S, p))).astype(model.np_dtype)
    dB = la.DeviceArray.from_host(model.device, B)
    pp = la.PosteriorPredictive(model, Xnew, ynew)
    r = pp.r
    L = model._L
    ev = Events(L, model.device)

    def ours():
        pp.reset()
        pp.update(dB)
    t_ours = repeats(ev.time, ours)
    table = pp.table()

    Xr = (X if Xnew is None else Xnew).astype(model.np_dtype)
    yr = y if Xnew is None else ynew
    dev = torch.device("cuda", model.device)
    Bt = torch.as_tensor(dB, device=dev)
    assert Bt.data_ptr() == dB.ptr  # the same buffer
    Xt = torch.as_tensor(Xr, device=dev)
    sgn = torch.as_tensor((2 * yr - 1).astype(model.np_dtype), device=dev)[None, :]
    chunk = max(1, min(S, (1 << 26) // r))

    def theirs():
        torch_table(torch, Bt, Xt, sgn, chunk)

    def ttime(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    t_torch = repeats(ttime, theirs)
    tt = torch_table(torch, Bt, Xt, sgn, chunk).cpu().numpy()
    agree = float(np.max(np.abs(tt[[0, 2, 3]] - table[[0, 2, 3]])))
    pairs = float(S) * r
    mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
    fl = floor_seconds(dtype, model_padded(p), pairs)
    line = (f"{name} {dtype}: S={S} r={r} p={p} pairs={pairs:.3e} | fused {mo * 1e3:.3f} ms (min {t_ours.min() * 1e3:.3f}, max {t_ours.max() * 1e3:.3f}, "
            f"n={len(t_ours)}) = {pairs / mo:.3e} pairs/s | torch {mt * 1e3:.3f} ms (min {t_torch.min() * 1e3:.3f}, max {t_torch.max() * 1e3:.3f}, n={len(t_torch)}, "
            f"chunk {chunk}) | torch / fused = {mt / mo:.2f} | VALU + transcendental issue floor {fl * 1e3:.3f} ms, share {fl / mo:.2f} | "
            f"max |fused - torch| on the mean rows {agree:.2e}")
    print(line, flush=True)
    lines.append(line)
    pp.close()
    dB.free()
    model.close()
    return mt / mo


def model_padded(p):
    return 4 if p <= 4 else 8 if p <= 8 else 16 if p <= 16 else 32 if p <= 32 else 64 if p <= 64 else 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the draw counts (a quick look)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()  # the yardstick needs its device: fail here, before any work, if torch finds none
    lines = [_lib.device_info(0)]
    print(lines[0], flush=True)
    X, y = la.load_pima()
    mp = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
    sd = np.array([1.71, 0.0655, 0.0068, 0.0184, 0.0226, 0.0429, 0.547, 0.0225]) * 0.3
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    ratios = []
    for dtype in ("float32", "float64"):
        ratios.append(shape("pima", X, y, ps, None, None, 4096 * 1000 // a.scale, dtype, mp, sd, lines))
    Xs, ys, bs = la.synthetic_logreg(4096, 128)
    Xn, yn, _ = la.synthetic_logreg(4096, 128, seed=5)
    ratios.append(shape("wide", Xs, ys, np.ones(128), Xn, yn, 1024 * 200 // a.scale, "float32", bs, 0.05, lines))
    Xt, yt, bt = la.synthetic_logreg(100000, 8)
    ratios.append(shape("tall", Xt, yt, np.ones(8), None, None, 1024 * 50 // a.scale, "float32", bt, 0.02, lines))
    verdict = f"slowest torch / fused ratio over the shapes: {min(ratios):.2f} (requirement: >= 1)"
    print(verdict)
    lines.append(verdict)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if min(ratios) >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
