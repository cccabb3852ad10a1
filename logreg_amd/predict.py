"""Posterior prediction, pointwise log predictive density and WAIC from the draws, on the device.

The samplers here produce draws faster than a host can take them; `PosteriorPredictive` consumes them where they are
(include/logreg_hip_predict.h, kernels in csrc/lr_predict.h).  Draws go in -- in any number of batches, as NumPy arrays or as the
`DeviceArray` blocks `ChainSet.advance` returns -- and a table `[5, r]` of float64 per-row statistics comes out:

    row 0  mean over draws of pi = sigma(x_i . beta)            the predictive probability P(y = 1 | x_i, data)
    row 1  sum of (pi - mean)^2                                 posterior sd of it = sqrt(row 1 / (S - 1))
    row 2  mean of L = sigma((2 y_i - 1) x_i . beta)            lppd_i = log(row 2)
    row 3  mean of l = log L
    row 4  sum of (l - mean)^2                                  p_waic,i = row 4 / (S - 1)

(rows 2 - 4 need labels and are NaN without).  WAIC as Gelman, Hwang & Vehtari (2014) and Vehtari, Gelman & Gabry (2017) define it:
elpd_waic = sum_i (lppd_i - p_waic,i), on the deviance scale waic = -2 elpd_waic.

    pp = PosteriorPredictive(model)                       # the model's own rows and labels
    res = mcmc(init, kern, iters=1000, summary_only=True, predictive=pp)   # no sample matrix anywhere
    pp.waic()["elpd_waic"]
    predict_proba(model, draws, X_new)                    # (mean, sd) for new rows from draws already on the host

There is no CPU path: without a GPU the constructor raises `LogregHipError` like everything else in this package.
`merge_predictive` (pure NumPy) combines the tables of chain shards or ranks, as `distributed.reduce_stats` does for the summaries.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._accum import ModelAccumulator
from ._lib import PRED_ROWS, check
from .model import LogReg


def waic_from_table(table, n_draws: int) -> dict:
    """WAIC from a table `[5, r]` of `n_draws` draws (any source: `PosteriorPredictive.table`, `merge_predictive`).
    -> elpd_waic, p_waic, se (= sqrt(r * var_i(elpd_i)), ddof = 1), waic = -2 elpd_waic, and the pointwise arrays lppd_i, p_waic_i,
    elpd_i."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != PRED_ROWS:
        raise ValueError(f"table must be [{PRED_ROWS}, r]; got {t.shape}")
    S = int(n_draws)
    if S < 2:
        raise ValueError(f"WAIC needs at least two draws (the variance of the log-likelihood); got {S}")
    if np.all(np.isnan(t[2])) and not np.all(np.isnan(t[0])):
        raise ValueError("this table has no labels (rows 2 - 4 are NaN): WAIC needs y")
    r = t.shape[1]
    lppd_i = np.log(t[2])
    p_i = t[4] / (S - 1)
    elpd_i = lppd_i - p_i
    elpd = float(np.sum(elpd_i))
    se = float(np.sqrt(r * np.var(elpd_i, ddof=1))) if r > 1 else float("nan")
    return {"elpd_waic": elpd, "p_waic": float(np.sum(p_i)), "se": se, "waic": -2.0 * elpd, "lppd": float(np.sum(lppd_i)),
            "lppd_i": lppd_i, "p_waic_i": p_i, "elpd_i": elpd_i, "n_draws": S}


def merge_predictive(tables, counts):
    """Tables `[5, r]` of disjoint sets of draws (chain shards, ranks, batches) with their draw counts -> (table, count) of the union,
    by the pairwise rule of Chan, Golub & LeVeque in the order given.  Pure NumPy; empty sets (count 0) are skipped."""
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    counts = [int(c) for c in counts]
    if len(tables) != len(counts) or not tables:
        raise ValueError("merge_predictive needs as many counts as tables, and at least one")
    shape = tables[0].shape
    if len(shape) != 2 or shape[0] != PRED_ROWS or any(t.shape != shape for t in tables):
        raise ValueError(f"every table must be [{PRED_ROWS}, r] with one r; got {[t.shape for t in tables]}")
    if any(c < 0 for c in counts):
        raise ValueError("counts must be >= 0")
    acc, n = np.full(shape, np.nan), 0
    for t, nb in zip(tables, counts):
        if nb == 0:
            continue
        if n == 0:
            acc, n = t.copy(), nb
            continue
        tot = n + nb
        w = nb / tot
        out = np.empty(shape)
        for mean, m2 in ((0, 1), (3, 4)):
            d = t[mean] - acc[mean]
            out[mean] = acc[mean] + d * w
            out[m2] = acc[m2] + t[m2] + d * d * (n * w)
        out[2] = acc[2] + (t[2] - acc[2]) * w
        acc, n = out, tot
    return acc, n


class PosteriorPredictive(ModelAccumulator):
    """Streaming accumulator of the posterior predictive of `model` at the rows `X_new` (None: the model's own design and labels,
    which are on the device already) with optional labels `y_new` in {0, 1}."""
    _prefix = "lr_predict"

    def __init__(self, model: LogReg, X_new=None, y_new=None):
        self._h = None
        _lib.load()
        _lib.require_gpu()  # no CPU path: without a device this raises LogregHipError whatever the arguments are
        if not isinstance(model, LogReg):
            raise TypeError(f"model must be a LogReg; got {type(model).__name__}")
        self.model = model
        self.has_labels = X_new is None or y_new is not None
        if X_new is None:
            if y_new is not None:
                raise ValueError("y_new without X_new: X_new=None means the model's own rows AND labels")
            X = y = None
            self.r = model.n
        else:
            X = np.ascontiguousarray(X_new, dtype=np.float64)
            if X.ndim != 2 or X.shape[1] != model.p:
                raise ValueError(f"X_new must be [r, p] with p={model.p}; got {X.shape}")
            if X.shape[0] == 0:
                raise ValueError("X_new has no rows")
            if not np.all(np.isfinite(X)):
                raise ValueError("X_new must be finite")
            self.r = X.shape[0]
            y = None
            if y_new is not None:
                y = np.ascontiguousarray(y_new, dtype=np.float64)
                if y.shape != (self.r,):
                    raise ValueError(f"y_new must be [r] = [{self.r}]; got {y.shape}")
                if not np.all((y == 0) | (y == 1)):
                    raise ValueError("y_new must hold 0 / 1 labels only")
        try:
            self._L = _lib.bind_predict(model._L)  # the accumulator belongs to the library handle that made the model
        except AttributeError as e:
            raise _lib.LogregHipError(f"the library behind this model has no prediction entry points (include/logreg_hip_predict.h): {e}") from e
        h = C.c_void_p()
        check(self._L.lr_predict_create(model.handle, X.ctypes.data if X is not None else None, y.ctypes.data if y is not None else None,
                                        self.r, C.byref(h)))
        self._h = h
        self.n_draws = 0

    def _library_count(self):
        n = C.c_int64()
        scratch = np.empty((PRED_ROWS, self.r), dtype=np.float64)
        return int(n.value) if self._L.lr_predict_result(self.handle, scratch.ctypes.data, C.byref(n)) == 0 else None

    def table(self) -> np.ndarray:
        """The table `[5, r]` (float64) of the draws so far; NaN everywhere before the first draw."""
        self.model.handle  # (raises if the model was closed, as update does)
        out = np.empty((PRED_ROWS, self.r), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_predict_result(self.handle, out.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return out

    def reset(self):
        check(self._L.lr_predict_reset(self.handle))
        self.n_draws = 0

    def proba(self):
        """(mean, sd) of the predictive probability per row; sd = posterior standard deviation (ddof = 1; NaN with one draw)."""
        t = self.table()
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = np.sqrt(t[1] / (self.n_draws - 1)) if self.n_draws > 1 else np.full(self.r, np.nan)
        return t[0], sd

    def lppd(self) -> np.ndarray:
        """Pointwise log predictive density log(mean_s p(y_i | beta_s)); needs labels."""
        if not self.has_labels:
            raise ValueError("lppd needs labels (y_new)")
        return np.log(self.table()[2])

    def waic(self) -> dict:
        if not self.has_labels:
            raise ValueError("WAIC needs labels (y_new)")
        return waic_from_table(self.table(), self.n_draws)

    def __repr__(self):
        return f"PosteriorPredictive(r={self.r}, labels={self.has_labels}, n_draws={self.n_draws}, {self.model!r})"


def predict_proba(model: LogReg, draws, X_new):
    """(mean, sd) of P(y = 1 | x, data) for the rows of `X_new` under the posterior `draws` ([S, p] or [iters, C, p])."""
    pp = PosteriorPredictive(model, X_new)
    try:
        return pp.update(draws).proba()
    finally:
        pp.close()


def waic(model: LogReg, draws) -> dict:
    """In-sample WAIC of `model` under the posterior `draws` (see `waic_from_table`)."""
    pp = PosteriorPredictive(model)
    try:
        return pp.update(draws).waic()
    finally:
        pp.close()
