#!/usr/bin/env python3
"""Times of the rank diagnostics (csrc/lr_rank.h) beside torch.sort + torch.searchsorted and beside the run that feeds them:
    python3 tools/rank_bench.py [--out FILE]     (needs the GPU; its lines are section 3 of profiles/r28_rank.txt; --out also writes them
                                                  to FILE)
    python3 tools/rank_bench.py --phases --only I (11 table() calls at shape I and nothing else: the program to put after
                                                  `rocprofv3 --kernel-trace --stats -d DIR --`, in a run of its own)
    python3 tools/rank_bench.py --read-trace DIR (the kernel times of that run by phase, from its *kernel_stats.csv; no GPU)
    python3 tools/rank_bench.py --resources      (registers and LDS of the kernels from the code objects; needs the object files, no GPU)

  whole     RankDiagnostics.table() (everything: two sorts, two rank passes, lag sums, the host finish) and .ranks(0) (one coordinate: keys,
            one sort, one rank pass, the copy back) on draws that are already on the device, between two HIP events, at
            4096 chains x 1000 kept x p = 8 float32 and 64 x 10 000 x p = 8 float64
  yardstick torch.sort + two torch.searchsorted (left, right) of the same draws as a [p, S] float64 tensor: the order and lo / hi alone,
            no transform, no fold, no sums -- what table() does twice (plain and folded) before its sums
  phases    kernel time by phase from a kernel trace: sort (k_rank_sort_tile + k_rank_merge_global), rank lookup (k_rank_lookup), transform
            (k_rank_transform), lag sums (k_rank_lag), the rest (gather, fold, quantiles, chain sums)
  run       mcmc(summary_only=True) of 4096 Pima chains with and without rank=, wall clock, result() included
One warm call, then 10 timed; the median is reported with the extremes.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import logreg_amd as la  # noqa: E402
from logreg_amd import _lib  # noqa: E402

RUNS = 10
SHAPES = [("many short chains", 4096, 1000, 8, "float32"), ("few long chains", 64, 10000, 8, "float64")]
PHASES = (("sort", ("k_rank_sort_tile", "k_rank_merge_global")), ("rank lookup", ("k_rank_lookup",)), ("transform", ("k_rank_transform",)), ("lag sums", ("k_rank_lag",)),
          ("the rest (gather, fold, quantiles, chain sums)", ("k_rank_gather", "k_rank_fold", "k_rank_quant", "k_rank_partial", "k_rank_final")))


def resources():
    from logreg_amd import build
    rows = [r for r in build.kernel_resources() if "k_rank_" in r["name"]]
    return [f"{r['name'].split('(')[0]}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['sgprs']} SGPRs, {r['lds']} bytes of LDS, {r['scratch']} bytes of scratch" for r in rows]


def hip_timer(L, device):
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.lr_event_create(device, C.byref(a)))
    _lib.check(L.lr_event_create(device, C.byref(b)))

    def timer(fn):
        ms = C.c_float()
        _lib.check(L.lr_event_record(device, a, None))
        fn()
        _lib.check(L.lr_event_record(device, b, None))
        _lib.check(L.lr_stream_sync(device, None))
        _lib.check(L.lr_event_elapsed_ms(device, a, b, C.byref(ms)))
        return ms.value * 1e-3
    return timer


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def median_of(timer, fn):
    timer(fn)  # warm
    t = np.array([timer(fn) for _ in range(RUNS)])
    return float(np.median(t)), float(t.min()), float(t.max())


def fmt(t, unit=1e3, what="ms"):
    return f"{t[0] * unit:.3f} {what} (min {t[1] * unit:.3f}, max {t[2] * unit:.3f})"


def draws(chains, steps, p, dtype, scale):
    """AR(1) chains, phi = 0.5, generated step by step so that no [steps, C, p] float64 temporary beyond the result is needed"""
    chains, steps = max(2, chains // scale), max(8, steps // scale)
    rng = np.random.default_rng(7)
    x = np.empty((steps, chains, p), dtype=dtype)
    cur = rng.standard_normal((chains, p))
    for t in range(steps):
        cur = 0.5 * cur + rng.standard_normal((chains, p))
        x[t] = cur
    return x


def filled(x):
    steps, chains, p = x.shape
    acc = la.RankDiagnostics(chains, p, steps, x.dtype)
    d = la.DeviceArray.from_host(acc.device, x)
    acc.update(d)
    acc.table()
    d.free()
    return acc


def whole(index, scale, lines):
    import torch
    name, chains, steps, p, dtype = SHAPES[index]
    x = draws(chains, steps, p, dtype, scale)
    steps, chains, p = x.shape
    S = steps // 2 * 2 * chains
    acc = filled(x)
    ht = hip_timer(acc._L, acc.device)
    t_all = median_of(ht, acc.table)
    t_one = median_of(ht, lambda: acc.ranks(0))
    res = acc.result()
    mine = acc.ranks(0)
    acc.free()
    flat = torch.from_numpy(np.ascontiguousarray(x[:steps // 2 * 2].reshape(S, p).T.astype(np.float64))).to(torch.device("cuda", 0))  # [p, S]

    def yardstick():
        s, _ = torch.sort(flat, dim=1)
        return torch.searchsorted(s, flat, right=False), torch.searchsorted(s, flat, right=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def torch_timer(fn):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3
    t_torch = median_of(torch_timer, yardstick)
    lo, hi = yardstick()
    same = bool(np.array_equal((lo[0] + hi[0] + 1).cpu().numpy().reshape(steps // 2 * 2, chains), mine))
    verdict = "" if t_all[0] <= 2 * t_torch[0] else "  -- the fused path LOSES to the yardstick here"
    line = (f"{name}: {chains} chains x {steps} kept x p={p} {x.dtype.name}, S = {S} per coordinate | table() {fmt(t_all)} = {t_all[0] / (p * S) * 1e9:.2f} ns per draw | "
            f"ranks(0) {fmt(t_one)} | torch.sort + 2 searchsorted of [p, S] float64 {fmt(t_torch)} | table() / yardstick = {t_all[0] / t_torch[0]:.2f} "
            f"(table() orders twice, plain and folded: table() / (2 x yardstick) = {t_all[0] / (2 * t_torch[0]):.2f}){verdict} | ranks equal torch's: {same} | "
            f"rhat max {np.nanmax(res['rhat']):.4f}, ess_bulk min {np.nanmin(res['ess_bulk']):.0f}, ess_tail min {np.nanmin(res['ess_tail']):.0f}, capped {int(np.nansum(res['capped_bulk']))}")
    print(line, flush=True)
    lines.append(line)


def phases(scale, only):
    for name, chains, steps, p, dtype in (SHAPES if only is None else [SHAPES[only]]):
        acc = filled(draws(chains, steps, p, dtype, scale))
        for _ in range(RUNS):
            acc.table()
        acc.free()


def read_trace(directory):
    """kernel time by phase from the *kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--phases --only I`: the totals over the
    run's 11 table() calls (one in `filled`, 10 more) divided by 11"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_stats.csv under {directory}")
    total = {}
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = next(v for k, v in row.items() if k.lower() == "name")
                ns = next(float(v) for k, v in row.items() if k.lower().startswith("totalduration"))
                total[name] = total.get(name, 0.0) + ns
    lines = []
    mine = sum(v for k, v in total.items() if "k_rank_" in k)
    for label, kernels in PHASES:
        ns = sum(v for k, v in total.items() if any(q in k for q in kernels))
        lines.append(f"phase {label}: {ns * 1e-6 / (RUNS + 1):.3f} ms per table() = {100 * ns / mine:.1f} % of the k_rank_ kernel time ({mine * 1e-6 / (RUNS + 1):.3f} ms)")
    return lines


def whole_run(lines, chains=4096, iters=100, thin=10):
    X, y = la.load_pima()
    ps = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    for dtype in ("float32", "float64"):
        model = la.LogReg(X, y, ps, dtype=dtype)
        beta, info = la.find_map(la.LogReg(X, y, ps, dtype="float64"))
        pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
        init = la.mcmc(np.tile(beta, (chains, 1)), kern, thin=thin, iters=100, verb=False, seed=2, summary_only=True)["state"]
        acc = la.RankDiagnostics(chains, 8, iters, dtype)

        def with_rank():
            acc.reset()
            return la.mcmc(init, kern, thin=thin, iters=iters, verb=False, seed=3, summary_only=True, rank=acc)
        t0 = median_of(wall, lambda: la.mcmc(init, kern, thin=thin, iters=iters, verb=False, seed=3, summary_only=True))
        t1 = median_of(wall, with_rank)
        tr = median_of(wall, acc.result)
        res = with_rank()
        line = (f"pima {dtype}, {chains} chains x {iters} kept (thin {thin}), HMC l = 20: run alone {fmt(t0)}, with rank= {fmt(t1)} "
                f"(+{(t1[0] / t0[0] - 1) * 100:.1f} %, result() included) | result() alone {fmt(tr)} | rank rhat max {np.max(res['rank']['rhat']):.4f} "
                f"(classical {np.max(res['rhat']):.4f}), ess_bulk min {np.min(res['rank']['ess_bulk']):.0f}, ess_tail min {np.min(res['rank']['ess_tail']):.0f}")
        print(line, flush=True)
        lines.append(line)
        acc.free()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--scale", type=int, default=1, help="divide the chain and step counts (a quick look)")
    ap.add_argument("--phases", action="store_true", help="only the result() calls, for a kernel trace")
    ap.add_argument("--only", type=int, default=None, help="with --phases: the index of the one shape to run")
    ap.add_argument("--read-trace", default=None, metavar="DIR", help="print the kernel times by phase of a traced --phases run and exit")
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers and LDS from the code objects and exit")
    a = ap.parse_args()
    if a.resources:
        print("\n".join(resources()))
        return 0
    if a.read_trace:
        print("\n".join(read_trace(a.read_trace)))
        return 0
    if a.phases:
        phases(a.scale, a.only)
        return 0
    import torch
    torch.cuda.init()  # the yardstick needs its device: fail here, before any work, if torch finds none
    lines = [_lib.device_info(0), f"median of {RUNS} calls after a warm one"]
    print(lines[0], flush=True)
    for index in range(len(SHAPES)):
        whole(index, a.scale, lines)
    whole_run(lines, chains=max(64, 4096 // a.scale))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
