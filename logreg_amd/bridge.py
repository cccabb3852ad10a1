"""Bridge sampling: the log marginal likelihood log p(y) = log INT exp(lpost) from the draws, on the device.

WAIC and PSIS-LOO judge predictive accuracy; Bayes factors and posterior model probabilities need the evidence.  `lpost` carries the
normalised prior, so the integral of exp(lpost) is p(y) itself.  `Bridge` evaluates, per draw and on the device, the float64 term
l = lpost - log g under a Gaussian proposal g = N(mean, cov) -- for the posterior draws it is fed (NumPy arrays or the `DeviceArray`
blocks `ChainSet.advance` returns) and for `n_proposal` draws of g it generates there -- and runs Meng & Wong's optimal bridge over the
two vectors of terms (include/logreg_hip_bridge.h states every step; kernels in csrc/lr_bridge.h):

    cov_acc = Covariance(chains, model.p, model.dtype, center, scale); mcmc(init, kern, iters=500, summary_only=True, covariance=cov_acc)
    acc = Bridge(model, *bridge_proposal(cov_acc.result()), max_draws=500 * chains)       # the proposal from a first half
    res = mcmc(state, kern, iters=500, summary_only=True, bridge=acc, autocorr=ac)        # the terms from the second
    acc.result(n_eff=res["autocorr"]["ess"].min())["logml"]
    bridge_sampling(model, draws, mean, cov)              # one shot from draws already on the host
    bridge_from_terms(l1, l2)                             # the iteration alone on any two vectors of terms (gathered shards of ranks)
    bridge_compare(a, b)                                  # the log Bayes factor of two results

The proposal should come from draws other than the ones the terms are computed from (Overstall & Forster 2010), as above, or from the
Laplace approximation: `bridge_proposal((beta_map, laplace_metric(model, beta_map)))`.  `n_eff` is the caller's: the effective size of
the posterior draws (`Autocorr`); it defaults to their number.  No warp-III or other non-Gaussian proposals.
There is no CPU path: without a GPU the constructor raises `LogregHipError` like everything else in this package.
`bridge_compare` and `bridge_proposal` are pure NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._accum import ModelAccumulator
from ._lib import BRIDGE_MAX_DRAWS, BRIDGE_ROWS, check
from .model import DeviceArray, LogReg

_NAMES = ("logml", "se", "iterations", "converged", "n_draws", "n_proposal", "n_eff", "n_nonfinite", "l1_min", "l1_max", "l2_min", "l2_max")


def bridge_from_table(table) -> dict:
    """The result dict of a table `[12]` (`Bridge.table`, `bridge_from_terms`): logml, se (the standard error of logml), iterations,
    converged, n_draws, n_proposal, n_eff (as used), n_nonfinite, and the ranges of the two vectors of terms."""
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (BRIDGE_ROWS,):
        raise ValueError(f"table must be [{BRIDGE_ROWS}]; got {t.shape}")
    r = {k: float(v) for k, v in zip(_NAMES, t)}
    for k in ("iterations", "n_draws", "n_proposal", "n_nonfinite"):
        r[k] = int(r[k]) if np.isfinite(r[k]) else 0
    r["converged"] = bool(t[3] == 1.0)
    r["table"] = t.copy()
    return r


def bridge_compare(a: dict, b: dict) -> dict:
    """Two `result()` dicts of two models of the same data -> log_bf = logml(a) - logml(b), the log Bayes factor of a against b, its
    standard error se = sqrt(se_a^2 + se_b^2) (independent runs), and the posterior probability of a under equal prior odds."""
    d = float(a["logml"]) - float(b["logml"])
    se = float(np.sqrt(float(a["se"]) ** 2 + float(b["se"]) ** 2))
    with np.errstate(over="ignore"):
        prob = float(1.0 / (1.0 + np.exp(-d))) if np.isfinite(d) else float("nan")
    return {"log_bf": d, "se": se, "prob_a": prob}


def bridge_proposal(x):
    """(mean [p], cov [p, p]) of the Gaussian proposal from a `Covariance` result (its pooled mean and covariance) or from a
    `(beta_map, inv_metric)` pair such as `(beta_map, laplace_metric(model, beta_map))`.  The covariance is symmetrised; it must be finite."""
    if isinstance(x, dict):
        mean, cov = x["mean"], x["cov"]
    else:
        try:
            mean, cov = x
        except (TypeError, ValueError):
            raise TypeError("bridge_proposal takes a Covariance result or a (mean, cov) pair") from None
    mean, cov = np.array(mean, dtype=np.float64), np.array(cov, dtype=np.float64)
    if mean.ndim != 1 or cov.shape != (mean.shape[0], mean.shape[0]):
        raise ValueError(f"mean must be [p] and cov [p, p]; got {mean.shape}, {cov.shape}")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))):
        raise ValueError("bridge_proposal needs a finite mean and covariance (a Covariance result needs at least two draws)")
    return mean, 0.5 * (cov + cov.T)


def _bind(L):
    try:
        return _lib.bind_bridge(L)
    except AttributeError as e:
        raise _lib.LogregHipError(f"the library behind this call has no bridge-sampling entry points (include/logreg_hip_bridge.h): {e}") from e


def _check_solve(n_eff, tol, maxit):
    n_eff = 0.0 if n_eff is None else float(n_eff)
    if n_eff != n_eff or (n_eff <= 0 and n_eff != 0.0):
        raise ValueError(f"n_eff must be positive (or None: the number of posterior draws); got {n_eff}")
    tol = float(tol)
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0; got {tol}")
    if isinstance(maxit, bool) or not isinstance(maxit, (int, np.integer)) or maxit < 0:
        raise ValueError(f"maxit must be a non-negative integer; got {maxit!r}")
    return n_eff, tol, int(maxit)


def _count(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer; got {type(v).__name__}")
    if v <= 0:
        raise ValueError(f"{name} must be positive; got {v}")
    if v > BRIDGE_MAX_DRAWS:
        raise ValueError(f"{name} = {v} is beyond the most an accumulator holds, {BRIDGE_MAX_DRAWS}")
    return int(v)


class Bridge(ModelAccumulator):
    """Accumulator of the bridge-sampling terms of `model` under up to `max_draws` posterior draws, against `n_proposal` (default
    `max_draws`) draws of the proposal N(mean, cov) generated on the device from `seed`."""
    _prefix = "lr_bridge"

    def __init__(self, model: LogReg, mean, cov, max_draws: int, n_proposal: int | None = None, seed: int = 0):
        self._h = None
        self.n_draws = 0
        _lib.load()
        _lib.require_gpu()  # no CPU path: without a device this raises LogregHipError whatever the arguments are
        if not isinstance(model, LogReg):
            raise TypeError(f"model must be a LogReg; got {type(model).__name__}")
        self.max_draws = _count("max_draws", max_draws)
        self.n_proposal = self.max_draws if n_proposal is None else _count("n_proposal", n_proposal)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64); got {seed!r}")
        mean, cov = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(cov, dtype=np.float64)
        if mean.shape != (model.p,) or cov.shape != (model.p, model.p):
            raise ValueError(f"mean must be [p] and cov [p, p] with p={model.p}; got {mean.shape}, {cov.shape}")
        if not np.all(np.isfinite(mean)):
            raise ValueError("mean must be finite")
        if not np.all(np.isfinite(cov)) or not np.allclose(cov, cov.T, rtol=1e-8, atol=1e-12 * float(np.max(np.abs(cov)))):
            raise ValueError("cov must be finite and symmetric")
        cov = np.ascontiguousarray(0.5 * (cov + cov.T))  # (symmetric within rounding, as an inverse Hessian comes: the library reads the lower triangle)
        self.model = model
        self.mean, self.cov, self.seed = mean.copy(), cov.copy(), int(seed)
        self._L = _bind(model._L)  # the accumulator belongs to the library handle that made the model
        h = C.c_void_p()
        rc = self._L.lr_bridge_create(model.handle, mean.ctypes.data, cov.ctypes.data, self.max_draws, self.n_proposal, self.seed, C.byref(h))
        if rc != 0:
            msg = (self._L.lr_last_error() or b"?").decode()
            if "positive definite" in msg or "not finite" in msg:  # the factorisation refused the matrix
                raise ValueError(f"cov is not a covariance matrix: {msg}")
            check(rc)
        self._h = h

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
        return int(n.value) if self._L.lr_bridge_terms(self.handle, None, None, C.byref(n), None) == 0 else None

    def check_run(self, chains, model, iters):
        """Raise ValueError unless this is an accumulator of `model` with room for the `iters` x `chains` draws of a run (`mcmc`, before
        anything runs)."""
        if self.model is not model:
            raise ValueError("bridge= must be a Bridge of the kernel's own model (its rows, prior, dtype and device)")
        need = self.n_draws + int(iters) * int(chains)
        if need > self.max_draws:
            raise ValueError(f"bridge= has max_draws = {self.max_draws}; this run brings its draws to {need}")

    def terms(self):
        """(l1 `[n_draws]`, l2 `[n_proposal]`): the float64 terms lpost - log g of the posterior draws, in arrival order, and of the
        proposal draws."""
        self.model.handle  # (raises if the model was closed, as update does)
        l1, l2 = np.empty(self.n_draws, dtype=np.float64), np.empty(self.n_proposal, dtype=np.float64)
        n1, n2 = C.c_int64(), C.c_int64()
        check(self._L.lr_bridge_terms(self.handle, l1.ctypes.data if l1.size else None, l2.ctypes.data, C.byref(n1), C.byref(n2)))
        assert (int(n1.value), int(n2.value)) == (self.n_draws, self.n_proposal)
        return l1, l2

    def proposal_draws(self) -> np.ndarray:
        """The proposal draws `[n_proposal, p]` in the model's dtype, regenerated on the device from (seed, j)."""
        self.model.handle
        out = np.empty((self.n_proposal, self.model.p), dtype=self.model.np_dtype)
        check(self._L.lr_bridge_proposal(self.handle, out.ctypes.data, None))
        return out

    def table(self, n_eff=None, tol=1e-10, maxit=1000) -> np.ndarray:
        """The table `[12]` (float64) of the terms so far; logml and se are NaN before the first draw."""
        n_eff, tol, maxit = _check_solve(n_eff, tol, maxit)
        self.model.handle
        out = np.empty(BRIDGE_ROWS, dtype=np.float64)
        check(self._L.lr_bridge_result(self.handle, n_eff, tol, maxit, out.ctypes.data))
        self.n_draws = int(out[4])
        return out

    def result(self, n_eff=None, tol=1e-10, maxit=1000) -> dict:
        """logml, se, iterations, converged, ...: see `bridge_from_table`.  `n_eff`: the effective size of the posterior draws (None:
        their number); the iteration stops at a change <= tol max(1, |logml|) or after `maxit` passes."""
        return bridge_from_table(self.table(n_eff, tol, maxit))

    def reset(self):
        """Forget the posterior draws; the proposal terms stay."""
        check(self._L.lr_bridge_reset(self.handle))
        self.n_draws = 0

    def __repr__(self):
        return f"Bridge(max_draws={self.max_draws}, n_proposal={self.n_proposal}, n_draws={self.n_draws}, seed={self.seed}, {self.model!r})"


def bridge_sampling(model: LogReg, draws, mean, cov, n_proposal=None, seed=0, n_eff=None, tol=1e-10, maxit=1000) -> dict:
    """The log marginal likelihood of `model` from the posterior `draws` ([S, p] or [iters, C, p]) and the proposal N(mean, cov); see
    `bridge_from_table`."""
    _lib.load()
    _lib.require_gpu()
    shape = draws.shape if isinstance(draws, DeviceArray) else np.shape(draws)
    if len(shape) not in (2, 3):
        raise ValueError(f"draws must be [S, p] or [iters, C, p]; got {tuple(shape)}")
    acc = Bridge(model, mean, cov, max(1, int(np.prod(shape[:-1], dtype=np.int64))), n_proposal=n_proposal, seed=seed)
    try:
        return acc.update(draws).result(n_eff=n_eff, tol=tol, maxit=maxit)
    finally:
        acc.close()


def bridge_from_terms(l1, l2, n_eff=None, tol=1e-10, maxit=1000, device: int = 0, stream=None) -> dict:
    """The iteration and the error alone: `l1` (posterior terms) and `l2` (proposal terms), 1-d float64 ndarrays or `DeviceArray`s (both
    of one kind) -> the result dict.  Needs no model: the gathered terms of several ranks go through this."""
    L = _bind(_lib.load())
    _lib.require_gpu()
    n_eff, tol, maxit = _check_solve(n_eff, tol, maxit)
    on_device = isinstance(l1, DeviceArray)
    if on_device != isinstance(l2, DeviceArray):
        raise ValueError("l1 and l2 must both be ndarrays or both be DeviceArrays")
    if on_device:
        if l1.dtype != np.float64 or l2.dtype != np.float64 or l1.device != l2.device:
            raise ValueError("DeviceArray terms must be float64 on one device")
        (n1, n2), p1, p2, device = (int(np.prod(l1.shape)), int(np.prod(l2.shape))), l1.ptr, l2.ptr, l1.device
    else:
        a1, a2 = np.ascontiguousarray(l1, dtype=np.float64), np.ascontiguousarray(l2, dtype=np.float64)
        if a1.ndim != 1 or a2.ndim != 1:
            raise ValueError(f"l1 and l2 must be 1-d; got {a1.shape}, {a2.shape}")
        n1, n2, p1, p2 = a1.size, a2.size, a1.ctypes.data, a2.ctypes.data
    if n1 == 0 or n2 == 0:
        raise ValueError("l1 and l2 must not be empty")
    out = np.empty(BRIDGE_ROWS, dtype=np.float64)
    check(L.lr_bridge_solve(int(device), p1, n1, p2, n2, n_eff, tol, maxit, int(on_device), out.ctypes.data, stream))
    return bridge_from_table(out)
