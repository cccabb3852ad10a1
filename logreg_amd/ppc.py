"""Posterior predictive checks from replicated outcomes, on the device.

WAIC, LOO and the evidence rank models against each other; none of them says whether a model is adequate, or where it is not.
`PredictiveCheck` (include/logreg_hip_ppc.h, kernels in csrc/lr_ppc.h) replicates the outcomes under every draw where the draws are --
y_rep(s, i) = [u < sigma(x_i . beta_s)], one counter-based uniform per (draw, row) pair -- and keeps what the checks of Gelman, Meng &
Stern (1996) and bayesplot's `ppc_stat_grouped` need:

    per group of rows g    the histogram of T_g = the number of ones among its replicates, against the observed count
    per draw               the realised discrepancy D = -2 log-likelihood of the observed and of the replicated outcomes
    per row                how often its replicate was 1

    pc = PredictiveCheck(model, groups=g)                 # the model's own rows and labels, rows labelled 0 .. G - 1
    res = mcmc(init, kern, iters=1000, summary_only=True, check=pc)["check"]
    res["p_two"]                                          # per group: is the observed count in the tails of its replicates?
    res.quantile(0.05), res.quantile(0.95)                # exact, from the histograms
    counts, dev, bits = pc.terms(draws)                   # per draw, to scatter-plot D_rep against D_obs

The same draws with the same seed give the same integer tables however they are cut into calls.  There is no CPU path: without a GPU
the constructor raises `LogregHipError` like everything else in this package.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._accum import ModelAccumulator
from ._lib import PPC_MAX_GROUPS, PPC_MOMENTS, check
from .model import DeviceArray, LogReg


class PpcResult(dict):
    """The result of a predictive check: a dict (see `ppc_from_table`) with `quantile`."""

    def quantile(self, q, rate=False):
        """Per group the `q`-quantile of the replicated count T_g (`rate=True`: of T_g / n_g), exact from the histogram: the smallest k
        with P(T_g <= k) >= q.  NaN before the first finite draw."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q must be in [0, 1]; got {q}")
        out = np.full(len(self["hist"]), np.nan)
        for g, h in enumerate(self["hist"]):
            n = int(h.sum())
            if n:
                out[g] = int(np.searchsorted(np.cumsum(h), max(1, int(np.ceil(q * n - 1e-9))), side="left"))
        with np.errstate(invalid="ignore", divide="ignore"):
            return out / self["n_g"] if rate else out


def ppc_from_table(hist, row_ones, counts, moments, t_obs, n_g, n_draws) -> PpcResult:
    """The result from the raw tables of include/logreg_hip_ppc.h (any source: `PredictiveCheck.tables()`, a file).
    -> per group (arrays [G]): n_g, t_obs, mean, sd (ddof = 1), p_ge = P(T_rep >= T_obs), p_le, p_two = min(1, 2 min(p_ge, p_le)) and
    rate_obs, rate_mean, rate_sd (T / n_g); `hist`: the G histograms; for the deviance dev_p = P(D_rep >= D_obs), dev_obs_mean,
    dev_obs_sd, dev_rep_mean, dev_rep_sd; row_freq [r]; n_draws, n_nonfinite, n (the finite draws, which every frequency is over); and
    the raw tables under "tables"."""
    n_g = np.asarray(n_g, dtype=np.int64).ravel()
    t_obs = np.asarray(t_obs, dtype=np.int64).ravel()
    hist = np.asarray(hist, dtype=np.uint64).ravel()
    row_ones = np.asarray(row_ones, dtype=np.uint64).ravel()
    counts = np.asarray(counts, dtype=np.uint64).ravel()
    moments = np.asarray(moments, dtype=np.float64).ravel()
    G = n_g.size
    if G < 1 or t_obs.size != G or hist.size != int(n_g.sum()) + G or row_ones.size != int(n_g.sum()) or counts.size != 2 or moments.size != PPC_MOMENTS:
        raise ValueError(f"tables do not fit together: {G} groups of {n_g.tolist()} rows, hist {hist.size}, row_ones {row_ones.size}, counts {counts.size}, "
                         f"moments {moments.size}")
    n_draws, bad = int(n_draws), int(counts[1])
    n = n_draws - bad
    off = np.concatenate([[0], np.cumsum(n_g + 1)])
    hs = [hist[off[g]:off[g + 1]].astype(np.int64) for g in range(G)]
    if any(int(h.sum()) != n for h in hs):
        raise ValueError(f"every histogram must hold the {n} finite draws; got {[int(h.sum()) for h in hs]}")
    mean, sd, p_ge, p_le = (np.full(G, np.nan) for _ in range(4))
    for g, h in enumerate(hs):
        if n == 0:
            continue
        k = np.arange(h.size, dtype=np.float64)
        mean[g] = float((k * h).sum()) / n
        if n > 1:
            sd[g] = np.sqrt(float((((k - mean[g]) ** 2) * h).sum()) / (n - 1))
        if t_obs[g] >= 0:
            p_ge[g], p_le[g] = float(h[t_obs[g]:].sum()) / n, float(h[:t_obs[g] + 1].sum()) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        ng = n_g.astype(np.float64)
        obs = np.where(t_obs >= 0, t_obs, np.nan).astype(np.float64)
        res = PpcResult(n_g=n_g, t_obs=t_obs, mean=mean, sd=sd, p_ge=p_ge, p_le=p_le, p_two=np.minimum(1.0, 2.0 * np.minimum(p_ge, p_le)),
                        rate_obs=obs / ng, rate_mean=mean / ng, rate_sd=sd / ng, hist=hs,
                        row_freq=row_ones.astype(np.float64) / n if n else np.full(row_ones.size, np.nan),
                        n_draws=n_draws, n_nonfinite=bad, n=n)
        labelled = bool(np.all(t_obs >= 0))
        res["dev_p"] = float(counts[0]) / n if n and labelled else float("nan")
        for name, k in (("dev_obs", 0), ("dev_rep", 2)):
            res[name + "_mean"] = float(moments[k])
            res[name + "_sd"] = float(np.sqrt(moments[k + 1] / (n - 1))) if n > 1 else float("nan")
    res["tables"] = dict(hist=hist, row_ones=row_ones, counts=counts, moments=moments, t_obs=t_obs, n_g=n_g, n_draws=n_draws)
    return res


class PredictiveCheck(ModelAccumulator):
    """Streaming posterior predictive check of `model` at the rows `X_new` (None: the model's own design and labels, which are on the
    device already) with optional labels `y_new` in {0, 1}, optional group labels `groups` [r] in 0 .. G - 1 (G = `n_groups`, or the
    largest label + 1; at most 32; None: one group) and a 64-bit `seed` of its own for the replicates."""
    _prefix = "lr_ppc"

    def __init__(self, model: LogReg, X_new=None, y_new=None, groups=None, seed=0, *, n_groups=None):
        self._h = None
        _lib.load()
        _lib.require_gpu()  # no CPU path: without a device this raises LogregHipError whatever the arguments are
        if not isinstance(model, LogReg):
            raise TypeError(f"model must be a LogReg; got {type(model).__name__}")
        self.model = model
        self.has_labels = X_new is None or y_new is not None
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise TypeError(f"seed must be an integer; got {type(seed).__name__}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64); got {seed}")
        self.seed = int(seed)
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
        g = None
        self.G = 1
        if groups is not None:
            ga = np.asarray(groups)
            if ga.shape != (self.r,):
                raise ValueError(f"groups must be [r] = [{self.r}]; got {ga.shape}")
            if ga.dtype.kind not in "iu" and not np.all(ga == np.floor(ga)):
                raise ValueError("groups must hold integer labels")
            if ga.min() < 0 or ga.max() >= PPC_MAX_GROUPS:
                raise ValueError(f"groups must be labels in 0 .. {PPC_MAX_GROUPS - 1}; got {ga.min()} .. {ga.max()}")
            g = np.ascontiguousarray(ga, dtype=np.int32)
            self.G = int(g.max()) + 1
        if n_groups is not None:
            if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not self.G <= n_groups <= PPC_MAX_GROUPS:
                raise ValueError(f"n_groups must be an integer in {self.G} .. {PPC_MAX_GROUPS} (the labels given reach {self.G - 1}); got {n_groups!r}")
            if groups is None and n_groups != 1:
                raise ValueError("n_groups without groups: groups=None means one group")
            self.G = int(n_groups)
        try:
            self._L = _lib.bind_ppc(model._L)  # the accumulator belongs to the library handle that made the model
        except AttributeError as e:
            raise _lib.LogregHipError(f"the library behind this model has no predictive-check entry points (include/logreg_hip_ppc.h): {e}") from e
        h = C.c_void_p()
        check(self._L.lr_ppc_create(model.handle, X.ctypes.data if X is not None else None, y.ctypes.data if y is not None else None, self.r,
                                    g.ctypes.data if g is not None else None, self.G, self.seed, C.byref(h)))
        self._h = h
        self.n_draws = 0

    def _library_count(self):
        n = C.c_int64()
        return int(n.value) if self._L.lr_ppc_result(self.handle, None, None, None, None, None, None, C.byref(n)) == 0 else None

    def check_run(self, chains, model, iters):
        """Raise ValueError unless this is an accumulator of `model` (`mcmc`, before anything runs)."""
        if self.model is not model:
            raise ValueError("check= must be a PredictiveCheck of the kernel's own model (its rows, dtype and device)")

    def tables(self) -> dict:
        """The raw tables of include/logreg_hip_ppc.h: hist [r + G], row_ones [r], counts [2] (uint64), moments [4], t_obs, n_g [G],
        n_draws -- what `ppc_from_table` takes."""
        self.model.handle  # (raises if the model was closed, as update does)
        hist, ones, counts = np.zeros(self.r + self.G, dtype=np.uint64), np.zeros(self.r, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        mom, t_obs, n_g, n = np.empty(PPC_MOMENTS), np.empty(self.G, dtype=np.int64), np.empty(self.G, dtype=np.int64), C.c_int64()
        check(self._L.lr_ppc_result(self.handle, hist.ctypes.data, ones.ctypes.data, counts.ctypes.data, mom.ctypes.data, t_obs.ctypes.data, n_g.ctypes.data,
                                    C.byref(n)))
        self.n_draws = int(n.value)
        return dict(hist=hist, row_ones=ones, counts=counts, moments=mom, t_obs=t_obs, n_g=n_g, n_draws=self.n_draws)

    def result(self) -> PpcResult:
        return ppc_from_table(**self.tables())

    def terms(self, draws, first_index=0, bits=True, stream=None):
        """The per-draw quantities of `draws` ([S, p] or [iters, C, p], an ndarray or a `DeviceArray`) taken as the draws of index
        `first_index`, `first_index` + 1, ...; nothing is accumulated.  -> counts [S, G] int32 (T_g), dev [S, 2] float64 (D_obs, D_rep)
        and the replicates [S, ceil(r / 32)] uint32, bit i & 31 of word i >> 5 for row i (None with `bits=False`)."""
        m = self.model
        m.handle
        shape = draws.shape if isinstance(draws, DeviceArray) else np.shape(draws)
        if len(shape) not in (2, 3) or shape[-1] != m.p:
            raise ValueError(f"draws must be [S, p] or [iters, C, p] with p={m.p}; got {tuple(shape)}")
        S = int(np.prod(shape[:-1], dtype=np.int64))
        if S == 0:
            raise ValueError("draws holds no draw (S = 0)")
        if isinstance(first_index, bool) or not isinstance(first_index, (int, np.integer)) or first_index < 0:
            raise ValueError(f"first_index must be an integer >= 0; got {first_index!r}")
        if isinstance(draws, DeviceArray):
            if draws.dtype != np.dtype(m.np_dtype) or draws.device != m.device:
                raise ValueError(f"a DeviceArray of draws must have the model's dtype {np.dtype(m.np_dtype).name} and device {m.device}; "
                                 f"got {draws.dtype.name} on device {draws.device}")
            ptr, on_device = draws.ptr, 1
        else:
            a = np.ascontiguousarray(draws, dtype=m.np_dtype)
            ptr, on_device = a.ctypes.data, 0
        counts, dev = np.empty((S, self.G), dtype=np.int32), np.empty((S, 2), dtype=np.float64)
        rep = np.empty((S, (self.r + 31) // 32), dtype=np.uint32) if bits else None
        check(self._L.lr_ppc_terms(self.handle, ptr, S, int(first_index), on_device, stream, counts.ctypes.data, dev.ctypes.data,
                                   rep.ctypes.data if bits else None))
        return counts, dev, rep

    def reset(self):
        check(self._L.lr_ppc_reset(self.handle))
        self.n_draws = 0

    def __repr__(self):
        return f"PredictiveCheck(r={self.r}, groups={self.G}, labels={self.has_labels}, seed={self.seed}, n_draws={self.n_draws}, {self.model!r})"
