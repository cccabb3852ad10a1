#!/usr/bin/env python3
"""Throughput of the posterior predictive check (csrc/lr_ppc.h) beside the prediction pass without a replicate and beside torch:
    python3 tools/ppc_bench.py [--out FILE]      (its lines are section 1 of profiles/r29_ppc.txt)

Shapes (draws S, check rows r, width p), those of tools/predict_bench.py:
    S = 4096 x 1000, r = 200 (Pima's own rows), p = 8, float32 and float64
    S = 1024 x 50,   r = n = 100 000 (the model's own rows), p = 8, float32
    S = 1024 x 200,  r = 4096, p = 128, float32
The draws are on the device before the clock starts.  Each shape: one warm call, then repeats timed one by one with HIP events until at
least 0.5 s of work has been timed (at least 5 repeats); medians.

Beside it:
    predict   PosteriorPredictive with labels on the same buffers: k_predict_partial + k_predict_merge, the same pass over the pairs
              without the replicate and without the reduction over the rows (csrc/lr_predict.h is untouched by the check)
    torch     what a user can do without the accumulator: bernoulli(sigmoid(B @ X.T)) on the same draws buffer, chunked so that a
              [chunk, r] matrix has at most 2^26 entries, with the same sums (the count of ones per draw and per row, the two deviances)
    run       a 4096-chain Pima HMC run (summary_only, 250 kept draws, thin 20) with and without check=, wall clock around mcmc"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402
from bench_util import Events, repeats_until as repeats  # noqa: E402


def torch_check(torch, Bt, Xt, yt, chunk):
    S, r = Bt.shape[0], Xt.shape[0]
    ones = torch.zeros(r, dtype=torch.int64, device=Bt.device)
    T = torch.empty(S, dtype=torch.int64, device=Bt.device)
    dev = torch.empty((S, 2), dtype=torch.float64, device=Bt.device)
    for a in range(0, S, chunk):
        eta = Bt[a:a + chunk] @ Xt.T
        rep = torch.bernoulli(torch.sigmoid(eta))
        ones += rep.sum(0, dtype=torch.int64)
        T[a:a + chunk] = rep.sum(1, dtype=torch.int64)
        l1, l0 = torch.nn.functional.logsigmoid(eta), torch.nn.functional.logsigmoid(-eta)
        dev[a:a + chunk, 0] = -2 * torch.where(yt > 0, l1, l0).sum(1, dtype=torch.float64)
        dev[a:a + chunk, 1] = -2 * torch.where(rep > 0, l1, l0).sum(1, dtype=torch.float64)
    return ones, T, dev


def shape(name, X, y, pscale, Xnew, ynew, S, dtype, center, spread, lines):
    import torch
    model = la.LogReg(X, y, pscale, dtype=dtype)
    rng = np.random.default_rng(1)
    p = X.shape[1]
    B = (center[None, :] + spread * rng.standard_normal((S, p))).astype(model.np_dtype)
    dB = la.DeviceArray.from_host(model.device, B)
    pc, pp = la.PredictiveCheck(model, Xnew, ynew, seed=1), la.PosteriorPredictive(model, Xnew, ynew)
    r = pc.r
    ev = Events(model._L, model.device)

    def ours():
        pc.reset()
        pc.update(dB)

    def predict():
        pp.reset()
        pp.update(dB)
    t_ours, t_pred = repeats(ev.time, ours), repeats(ev.time, predict)
    res = pc.result()

    Xr = (X if Xnew is None else Xnew).astype(model.np_dtype)
    yr = y if Xnew is None else ynew
    dev = torch.device("cuda", model.device)
    Bt = torch.as_tensor(dB, device=dev)
    assert Bt.data_ptr() == dB.ptr  # the same buffer
    Xt, yt = torch.as_tensor(Xr, device=dev), torch.as_tensor(yr.astype(model.np_dtype), device=dev)[None, :]
    chunk = max(1, min(S, (1 << 26) // r))

    def ttime(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    t_torch = repeats(ttime, lambda: torch_check(torch, Bt, Xt, yt, chunk))
    _, T, _ = torch_check(torch, Bt, Xt, yt, chunk)
    pairs = float(S) * r
    mo, mp, mt = (float(np.median(t)) for t in (t_ours, t_pred, t_torch))
    line = (f"{name} {dtype}: S={S} r={r} p={p} pairs={pairs:.3e} | check {mo * 1e3:.3f} ms (min {t_ours.min() * 1e3:.3f}, max {t_ours.max() * 1e3:.3f}, n={len(t_ours)}) = "
            f"{pairs / mo:.3e} pairs/s | predict {mp * 1e3:.3f} ms (n={len(t_pred)}): check / predict = {mo / mp:.2f} | torch {mt * 1e3:.3f} ms (n={len(t_torch)}, chunk {chunk}): "
            f"torch / check = {mt / mo:.2f} | mean T_rep {res['mean'][0]:.2f} (torch's own replicates {float(T.double().mean()):.2f}), observed {res['t_obs'][0]}, "
            f"P(D_rep >= D_obs) {res['dev_p']:.3f}")
    print(line, flush=True)
    lines.append(line)
    pc.close()
    pp.close()
    dB.free()
    model.close()


def run_share(lines, chains=4096, iters=250, thin=20):
    X, y = la.load_pima()
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    pre = np.array([100., 1., 1., 1., 1., 1., 25., 1.])
    mp = np.array([-9.19131622, 0.09705401, 0.03112265, -0.00564495, -0.00062272, 0.0814371, 1.26032561, 0.03939102])
    for dtype in ("float32", "float64"):
        model = la.LogReg(X, y, ps, dtype=dtype)
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre)
        init = np.tile(mp, (chains, 1))
        pc = la.PredictiveCheck(model, seed=1)
        times = {False: [], True: []}
        for rep in range(6):  # (the first pair warms up)
            for with_check in (False, True):
                pc.reset()
                t0 = time.perf_counter()
                la.mcmc(init, kern, thin=thin, iters=iters, verb=False, summary_only=True, seed=2, check=pc if with_check else None)
                if rep:
                    times[with_check].append(time.perf_counter() - t0)
        a, b = float(np.median(times[False])), float(np.median(times[True]))
        line = (f"run {dtype}: {chains} chains x {iters} kept (thin {thin}), Pima | without check {a * 1e3:.1f} ms, with check= {b * 1e3:.1f} ms (medians of 5): "
                f"+{(b / a - 1) * 100:.1f} %")
        print(line, flush=True)
        lines.append(line)
        pc.close()
        model.close()


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
    for dtype in ("float32", "float64"):
        shape("pima", X, y, ps, None, None, 4096 * 1000 // a.scale, dtype, mp, sd, lines)
    Xt, yt, bt = la.synthetic_logreg(100000, 8)
    shape("tall", Xt, yt, np.ones(8), None, None, 1024 * 50 // a.scale, "float32", bt, 0.02, lines)
    Xs, ys, bs = la.synthetic_logreg(4096, 128)
    Xn, yn, _ = la.synthetic_logreg(4096, 128, seed=5)
    shape("wide", Xs, ys, np.ones(128), Xn, yn, 1024 * 200 // a.scale, "float32", bs, 0.05, lines)
    run_share(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
