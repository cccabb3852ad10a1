"""PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation from the draws, on the device.

Vehtari, Gelman & Gabry (2017) recommend PSIS-LOO over WAIC: the same cost class, more robust, and with a per-observation diagnostic,
the Pareto shape k-hat, that says when the estimate cannot be trusted (k-hat > 0.7).  `PsisLoo` keeps the pointwise log-likelihood
matrix of the model's own rows on the device (include/logreg_hip_loo.h, kernels in csrc/lr_loo.h), fills it from draws -- NumPy arrays
or the `DeviceArray` blocks `ChainSet.advance` returns -- and reduces it there to a table `[5, n]` of float64:

    row 0  elpd_loo_i      row 1  khat_i      row 2  n_eff_i (of the smoothed weights)      row 3  lppd_i      row 4  n_tail_i

    acc = PsisLoo(model, max_draws=1000 * 64)
    res = mcmc(init, kern, iters=1000, summary_only=True, loo=acc)      # no sample matrix and no [S, n] matrix on the host
    res["loo"]["elpd_loo"], res["loo"]["n_khat_over_0_7"]
    psis_loo(model, draws)                                # one shot from draws already on the host, as waic(model, draws)
    psis_from_loglik(loglik)                              # the PSIS stage alone on any [S, r] matrix (gathered shards of ranks)

The relative efficiency of the draws is taken as r_eff = 1: `n_eff` is that of independent draws, and no correction for the
autocorrelation of a chain enters the tail length.  No moment matching or refits for high k-hat.
There is no CPU path: without a GPU the constructor raises `LogregHipError` like everything else in this package.
`loo_from_table` and `loo_compare` are pure NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._accum import ModelAccumulator
from ._lib import LOO_MAX_DRAWS, LOO_ROWS, check
from .model import DeviceArray, LogReg


def tail_length(S: int) -> int:
    """M = min(floor(S / 5), m3), m3 the smallest integer with m3^2 >= 9 S: the most draws PSIS smooths, in integers."""
    import math
    S = int(S)
    if S <= 0:
        return 0
    m3 = math.isqrt(9 * S)
    if m3 * m3 < 9 * S:
        m3 += 1
    return min(S // 5, m3)


def loo_from_table(table, n_draws: int) -> dict:
    """The summary of a table `[5, n]` of `n_draws` draws (`PsisLoo.table`, `psis_from_loglik`): elpd_loo, p_loo = sum(lppd_i -
    elpd_i), se = sqrt(n var(elpd_i, ddof = 1)), looic = -2 elpd_loo, the pointwise arrays elpd_i, khat, n_eff, lppd_i, n_tail, n_draws,
    and n_khat_over_0_7, the number of observations whose estimate should not be trusted."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != LOO_ROWS:
        raise ValueError(f"table must be [{LOO_ROWS}, n]; got {t.shape}")
    n = t.shape[1]
    elpd_i, khat, n_eff, lppd_i = t[0].copy(), t[1].copy(), t[2].copy(), t[3].copy()
    elpd = float(np.sum(elpd_i))
    se = float(np.sqrt(n * np.var(elpd_i, ddof=1))) if n > 1 else float("nan")
    with np.errstate(invalid="ignore"):
        over = int(np.sum(khat > 0.7))
    return {"elpd_loo": elpd, "p_loo": float(np.sum(lppd_i - elpd_i)), "se": se, "looic": -2.0 * elpd, "elpd_i": elpd_i, "khat": khat,
            "n_eff": n_eff, "lppd_i": lppd_i, "n_tail": t[4].copy(), "n_draws": int(n_draws), "n_khat_over_0_7": over}


def loo_compare(a: dict, b: dict) -> dict:
    """Two `result()` dicts over the same observations -> elpd_diff = elpd_loo(a) - elpd_loo(b) and its standard error
    se_diff = sqrt(n var(elpd_i^a - elpd_i^b, ddof = 1))."""
    ea, eb = np.asarray(a["elpd_i"], dtype=np.float64), np.asarray(b["elpd_i"], dtype=np.float64)
    if ea.ndim != 1 or ea.shape != eb.shape:
        raise ValueError(f"loo_compare needs the same observations on both sides; got n = {ea.shape} and {eb.shape}")
    n = ea.shape[0]
    d = ea - eb
    return {"elpd_diff": float(np.sum(d)), "se_diff": float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else float("nan"), "n": n}


def _bind(L):
    try:
        return _lib.bind_loo(L)
    except AttributeError as e:
        raise _lib.LogregHipError(f"the library behind this call has no PSIS-LOO entry points (include/logreg_hip_loo.h): {e}") from e


class PsisLoo(ModelAccumulator):
    """Accumulator of the pointwise log-likelihood of `model`'s own rows under up to `max_draws` draws, and its PSIS-LOO summary."""
    _prefix = "lr_loo"

    def __init__(self, model: LogReg, max_draws: int):
        self._h = None
        _lib.load()
        _lib.require_gpu()  # no CPU path: without a device this raises LogregHipError whatever the arguments are
        if not isinstance(model, LogReg):
            raise TypeError(f"model must be a LogReg; got {type(model).__name__}")
        if isinstance(max_draws, bool) or not isinstance(max_draws, (int, np.integer)):
            raise TypeError(f"max_draws must be an integer; got {type(max_draws).__name__}")
        if max_draws <= 0:
            raise ValueError(f"max_draws must be positive; got {max_draws}")
        self.model = model
        self.n = model.n
        self.max_draws = int(max_draws)
        self._L = _bind(model._L)  # the accumulator belongs to the library handle that made the model
        h = C.c_void_p()
        check(self._L.lr_loo_create(model.handle, self.max_draws, C.byref(h)))
        self._h = h
        self.n_draws = 0

    @property
    def dtype(self):
        return np.dtype(self.model.np_dtype)

    @property
    def device(self):
        return self.model.device

    def _check_room(self, S):
        if self.n_draws + S > self.max_draws:
            raise ValueError(f"{self.n_draws} draws held + {S} more exceed max_draws = {self.max_draws}")

    def _library_count(self):
        n = C.c_int64()
        return int(n.value) if self._L.lr_loo_loglik(self.handle, None, C.byref(n)) == 0 else None

    def check_run(self, chains, model, iters):
        """Raise ValueError unless this is an accumulator of `model` with room for the `iters` x `chains` draws of a run (`mcmc`, before
        anything runs)."""
        if self.model is not model:
            raise ValueError("loo= must be a PsisLoo of the kernel's own model (its rows, dtype and device)")
        need = self.n_draws + int(iters) * int(chains)
        if need > self.max_draws:
            raise ValueError(f"loo= has max_draws = {self.max_draws}; this run brings its draws to {need}")

    def loglik(self) -> np.ndarray:
        """The pointwise log-likelihood `[S, n]` in the model's dtype, in arrival order -- what arviz-style tools take."""
        self.model.handle
        out = np.empty((self.n_draws, self.n), dtype=self.model.np_dtype)
        n = C.c_int64()
        check(self._L.lr_loo_loglik(self.handle, out.ctypes.data if out.size else None, C.byref(n)))
        assert int(n.value) == self.n_draws
        return out

    def table(self) -> np.ndarray:
        """The table `[5, n]` (float64) of the draws so far; NaN everywhere before the first draw."""
        self.model.handle  # (raises if the model was closed, as update does)
        out = np.empty((LOO_ROWS, self.n), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_loo_result(self.handle, out.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return out

    def result(self) -> dict:
        return loo_from_table(self.table(), self.n_draws)

    def reset(self):
        check(self._L.lr_loo_reset(self.handle))
        self.n_draws = 0

    def __repr__(self):
        return f"PsisLoo(n={self.n}, max_draws={self.max_draws}, n_draws={self.n_draws}, {self.model!r})"


def psis_loo(model: LogReg, draws) -> dict:
    """In-sample PSIS-LOO of `model` under the posterior `draws` ([S, p] or [iters, C, p]; see `loo_from_table`)."""
    _lib.load()
    _lib.require_gpu()
    shape = draws.shape if isinstance(draws, DeviceArray) else np.shape(draws)
    if len(shape) not in (2, 3):
        raise ValueError(f"draws must be [S, p] or [iters, C, p]; got {tuple(shape)}")
    acc = PsisLoo(model, max(1, int(np.prod(shape[:-1], dtype=np.int64))))
    try:
        return acc.update(draws).result()
    finally:
        acc.close()


def psis_from_loglik(loglik, device: int = 0, stream=None) -> np.ndarray:
    """The PSIS stage alone: `loglik` `[S, r]` (ndarray: float32 stays float32, everything else becomes float64; or a `DeviceArray` of
    either) -> the table `[5, r]` of float64.  Needs no model."""
    L = _bind(_lib.load())
    _lib.require_gpu()
    on_device = isinstance(loglik, DeviceArray)
    if on_device:
        shape, dt, ptr, device = loglik.shape, loglik.dtype, loglik.ptr, loglik.device
    else:
        a = np.asarray(loglik)
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        shape, dt, ptr = a.shape, a.dtype, a.ctypes.data
    if len(shape) != 2 or shape[0] == 0 or shape[1] == 0:
        raise ValueError(f"loglik must be [S, r] with S, r > 0; got {tuple(shape)}")
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"loglik must be float32 or float64; got {dt.name}")
    out = np.empty((LOO_ROWS, shape[1]), dtype=np.float64)
    check(L.lr_psis(int(device), ptr, shape[0], shape[1], _lib.LR_F32 if dt == np.float32 else _lib.LR_F64, int(on_device), out.ctypes.data, stream))
    return out
