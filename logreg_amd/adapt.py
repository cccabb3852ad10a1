"""Warm-up for `nutsKernel`: Stan-style windowed adaptation of one step size and one diagonal metric, pooled over all chains, on the device.

The reference's NumPyro script runs `MCMC(kernel, num_warmup=1000, ...)` (`Python/fit-numpyro.py:44`); `nuts_warmup` is that warm-up for the
fused sampler (include/logreg_hip_adapt.h states the definition; kernels in csrc/lr_nuts.h and csrc/lr_adapt.h):

    res = nuts_warmup(model.lpost, model.glp, init, num_warmup=1000)      # from eps = 1 and the unit metric
    out = mcmc(res.state, res.kernel, thin=1, iters=1000)                 # res.kernel = nutsKernel(lpost, glp, res.eps, res.dmm, max_depth)

Every iteration the mean acceptance statistic of all C chains drives one dual-averaging step of the shared step size, and in the slow
windows the states of all chains enter one pooled variance per coordinate: 4096 chains give both with almost no noise.  The W iterations
are enqueued back to back, with no host round trip.  The result depends on the chain count: a shard of a larger run (`mcmc_sharded`)
adapts by itself; pooling across ranks is not built.  There is no CPU path.

Tall and wide models (rows beyond the LDS, or 32 < p <= 128) sample on the stepwise engine (`mcmc(..., mode="stepwise")`); their warm-up is
`nuts_warmup_stepwise(...)` (include/logreg_hip_adapt_tall.h): the same adaptation, the iterations as that engine's launches.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import AdaptInfo, AdaptOpts, RunOpts, check
from .kernels import NUTS_COUNTERS, _inv_metric_array, _model_of, nutsKernel

TRACE_COLUMNS = ("eps", "accept_stat", "log_eps_bar", "window", "n")


def adapt_schedule(num_warmup, init_buffer=0, term_buffer=0, base_window=0):
    """-> (first iteration of the first window, [exclusive window ends]) of a warm-up of `num_warmup` iterations (`lr_adapt_schedule`:
    host code, no device).  Buffers: 0 = Stan's defaults 75, 50, 25."""
    L = _adapt_library()
    ends = (C.c_int32 * _lib.ADAPT_MAX_WINDOWS)()
    n, init = C.c_int32(), C.c_int32()
    check(L.lr_adapt_schedule(int(num_warmup), int(init_buffer), int(term_buffer), int(base_window), ends, C.byref(n), C.byref(init)))
    return int(init.value), [int(e) for e in ends[:n.value]]


def _adapt_library(L=None):
    L = _lib.load() if L is None else L
    try:
        return _lib.bind_adapt(L)
    except AttributeError as e:
        raise _lib.LogregHipError(f"this library has no warm-up entry points (include/logreg_hip_adapt.h): {e}") from e


def _adapt_tall_library(L=None):
    L = _lib.load() if L is None else L
    try:
        return _lib.bind_adapt_tall(L)
    except AttributeError as e:
        raise _lib.LogregHipError(f"this library has no stepwise warm-up entry points (include/logreg_hip_adapt_tall.h): {e}") from e


def _dense_library(L=None):
    L = _lib.load() if L is None else L
    try:
        return _lib.bind_dense(_lib.bind_adapt(L))
    except AttributeError as e:
        raise _lib.LogregHipError(f"this library has no dense-metric entry points (include/logreg_hip_dense.h): {e}") from e


def _warmup(who, symbols, mode, library, start, shapes, finish, lpost, glp, init, num_warmup, target_accept, eps, max_depth, adapt_metric, seed, chain_offset,
            keep):
    """The body of `nuts_warmup` and `nuts_warmup_dense`: the checks, the start state and the seed, create / run / result / trace / destroy
    and the result.  What differs comes as arguments: `who` names the caller in the error text, `symbols` are the prefixes of the entry
    points in the binding `library` (create and run; result, trace and destroy), `mode` is the launch mode of the run (`_lib.MODE_*`), `start(p)` checks the start metric and returns (`AdaptOpts.dmm0` or None, the further array
    arguments of create), `shapes(p)` the shapes of the metric and of a window's row of `metric_trace`, `finish(res, metric, max_depth)`
    adds the metric and the `kernel` to the result."""
    model = _model_of(lpost, "lpost")
    if model is None or _model_of(glp, "glp") is not model:
        raise ValueError(f"{who} needs a fused kernel: lpost and glp must be the closures of one LogReg (the generic NumPy NUTS has no warm-up)")
    W, max_depth = int(num_warmup), int(max_depth)
    if W < 1:
        raise ValueError(f"num_warmup must be >= 1, got {num_warmup}")
    if not 1 <= max_depth <= _lib.NUTS_MAX_DEPTH:
        raise ValueError(f"max_depth must be in 1..{_lib.NUTS_MAX_DEPTH}, got {max_depth}")
    if not 0.0 < float(target_accept) < 1.0:
        raise ValueError(f"target_accept must be in (0, 1), got {target_accept}")
    if not (np.isfinite(eps) and float(eps) > 0):
        raise ValueError(f"eps must be finite and > 0, got {eps}")
    p = model.p
    dmm0, more = start(p)
    st = np.array(np.atleast_2d(np.asarray(init, dtype=np.float64)), dtype=model.np_dtype, order="C")
    if st.ndim != 2 or st.shape[1] != p:
        raise ValueError(f"init must be [p] or [C,p] with p={p}; got {np.shape(init)}")
    Cn = st.shape[0]
    L = library(model._L)  # the library that made the model
    make, read = symbols
    _lib.require_gpu()
    if seed is None:
        seed = int(np.random.randint(0, 2**31 - 1))
    seed = int(seed)
    o = AdaptOpts(W=W, adapt_metric=int(bool(adapt_metric)), delta=float(target_accept), eps0=float(eps), dmm0=None if dmm0 is None else dmm0.ctypes.data)
    h = C.c_void_p()
    check(getattr(L, make + "_create")(model.handle, Cn, C.byref(o), *(a.ctypes.data for a in more), C.byref(h)))
    try:
        counters = np.zeros(Cn, dtype=NUTS_COUNTERS)
        draws = np.empty((W, Cn, p), dtype=model.np_dtype) if keep else None
        opts = RunOpts(n_chains=Cn, chain_offset=int(chain_offset), thin=1, iters=1, seed=seed & 0xFFFFFFFFFFFFFFFF, group=0, mode=mode, on_device=0)
        check(getattr(L, make + "_run")(h, st.ctypes.data, W, max_depth, C.byref(opts), draws.ctypes.data if keep else None, counters.ctypes.data, None, None))
        e, info = C.c_double(), AdaptInfo()
        metric_shape, row_shape = shapes(p)
        metric = np.empty(metric_shape, dtype=np.float64)
        check(getattr(L, read + "_result")(h, C.byref(e), metric.ctypes.data, C.byref(info)))
        trace = np.zeros((W, _lib.ADAPT_TRACE_COLS), dtype=np.float64)
        metric_trace = np.zeros((info.n_windows, *row_shape), dtype=np.float64)
        check(getattr(L, read + "_trace")(h, trace.ctypes.data, metric_trace.ctypes.data if info.n_windows else None))
    finally:
        getattr(L, read + "_destroy")(h)
    res = SimpleNamespace(eps=float(e.value), state=st.astype(np.float64), trace=trace, metric_trace=metric_trace,
                          info={"n_leapfrog": counters["n_leapfrog"].astype(np.int64), "divergent": counters["divergent"].astype(np.int64),
                                "max_depth_hits": counters["max_depth_hits"].astype(np.int64), "mean_depth": counters["depth_sum"] / W,
                                "mean_accept_stat": counters["accept_stat_sum"] / W, "metric_skipped": int(info.metric_skipped),
                                "windows": int(info.windows), "iterations": int(info.iterations), "seed": seed})
    finish(res, metric, max_depth)
    if keep:
        res.draws = draws
    return res


def _nuts_warmup(who, mode, lpost, glp, init, num_warmup, target_accept, eps, dmm, max_depth, adapt_metric, seed, chain_offset, keep):
    """`nuts_warmup` (`mode` "auto") and `nuts_warmup_stepwise` ("stepwise"): the diagonal metric's start and finish; the engine as data"""
    def start(p):
        dmm0 = np.ascontiguousarray(np.broadcast_to(np.asarray(dmm, dtype=np.float64), (p,)))
        if not np.all(np.isfinite(dmm0) & (dmm0 > 0)):
            raise ValueError("dmm must be finite and > 0")
        return dmm0, ()

    def finish(res, dm, depth):
        res.dmm, res.pre, res.kernel = dm, 1.0 / dm, nutsKernel(lpost, glp, res.eps, dm, depth)
    tall = mode == "stepwise"
    return _warmup(who, ("lr_tall_adapt" if tall else "lr_adapt", "lr_adapt"), _lib.MODE_BY_NAME[mode], _adapt_tall_library if tall else _adapt_library, start,
                   lambda p: ((p,), (2, p)), finish, lpost, glp, init, num_warmup, target_accept, eps, max_depth, adapt_metric, seed, chain_offset, keep)


def nuts_warmup(lpost, glp, init, num_warmup=1000, *, target_accept=0.8, eps=1.0, dmm=1, max_depth=10, adapt_metric=True, seed=None,
                chain_offset=0, keep=False):
    """Run `num_warmup` adaptation iterations of all chains of `init` (`[p]` or `[C, p]`) and return the adapted sampler.

    Returns an object with `eps`, `dmm`, `pre` (= 1 / dmm: BlackJAX's inverse mass matrix), `state` `[C, p]`, `kernel`
    (`nutsKernel(lpost, glp, eps, dmm, max_depth)`, ready for `mcmc`), `trace` `[W, 5]` (columns `TRACE_COLUMNS`), `metric_trace`
    `[windows, 2, p]` (var, dmm per window), `info` (the per-chain counters as `ChainSet.nuts_info` gives them, and `metric_skipped`,
    `windows`, `seed`) and, with `keep=True`, `draws` `[W, C, p]`.  `lpost` and `glp` must be the closures of one `LogReg`."""
    return _nuts_warmup("nuts_warmup", "auto", lpost, glp, init, num_warmup, target_accept, eps, dmm, max_depth, adapt_metric, seed, chain_offset, keep)


def nuts_warmup_stepwise(lpost, glp, init, num_warmup=1000, *, target_accept=0.8, eps=1.0, dmm=1, max_depth=10, adapt_metric=True, seed=None,
                         chain_offset=0, keep=False):
    """`nuts_warmup` on the stepwise engine (include/logreg_hip_adapt_tall.h), for the models `mcmc(..., mode="stepwise")` samples -- 32 < p
    <= 128, or rows beyond the LDS -- and only for those (a shape of the fused kernel is refused, with the hint to `nuts_warmup`).  The
    same arguments, the same result; run it with `mcmc(res.state, res.kernel, mode="stepwise")`.  The host waits on the device at the end of
    every tree doubling, as that sampling run does.  A function of its own, as `nuts_warmup_dense` is: `nuts_warmup`'s parameter list is
    pinned by its tests."""
    return _nuts_warmup("nuts_warmup_stepwise", "stepwise", lpost, glp, init, num_warmup, target_accept, eps, dmm, max_depth, adapt_metric, seed, chain_offset, keep)


def nuts_warmup_dense(lpost, glp, init, num_warmup=1000, *, target_accept=0.8, eps=1.0, inv_metric=None, max_depth=10, adapt_metric=True, seed=None,
                      chain_offset=0, keep=False):
    """`nuts_warmup` for the DENSE metric (include/logreg_hip_dense.h "Warm-up"; Stan's metric=dense_e, NumPyro's dense_mass=True): the
    windows pool one p x p covariance over chains and time and the sampler gets the full inverse metric.  It starts from `inv_metric`
    (`[p, p]`, default the unit matrix); with `adapt_metric=False` only the step size is tuned to that fixed matrix -- what a metric
    from elsewhere (`optimize.laplace_metric`, `covariance.dense_metric`) needs.

    Returns what `nuts_warmup` returns with `inv_metric` `[p, p]` in place of `dmm` / `pre`, `metric_trace` `[windows, p, p]` (the
    matrix after each window) and a dense `kernel` (`nutsKernel(lpost, glp, eps, max_depth=, inv_metric=res.inv_metric)`);
    `info["metric_skipped"]` counts the windows whose matrix was not positive definite (the previous one stays)."""
    def start(p):
        sig0 = np.eye(p) if inv_metric is None else _inv_metric_array(inv_metric, p)
        if not np.all(np.isfinite(np.tril(sig0))):
            raise ValueError("inv_metric must be finite")
        return None, (sig0,)

    def finish(res, sig, depth):
        res.inv_metric, res.kernel = sig, nutsKernel(lpost, glp, res.eps, max_depth=depth, inv_metric=sig)
    return _warmup("nuts_warmup_dense", ("lr_dense_adapt", "lr_dense_adapt"), _lib.MODE_AUTO, _dense_library, start, lambda p: ((p, p), (p, p)), finish, lpost, glp, init, num_warmup, target_accept,
                   eps, max_depth, adapt_metric, seed, chain_offset, keep)
