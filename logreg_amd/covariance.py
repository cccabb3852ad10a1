"""Posterior covariance and correlation of the kept draws, on the device.

The reference's analysis of a run (`Python/analyse.R:16-18`) looks at `cor(out)` after `mcmcSummary(out)`: the joint structure of the
posterior, which needs the whole `[iters, C, p]` matrix on the host.  `Covariance` is the streaming accumulator for it
(include/logreg_hip_cov.h, kernels in csrc/lr_cov.h): blocks `[k, C, p]` in time order go in -- NumPy arrays or the `DeviceArray` blocks
`ChainSet.advance` returns, from any sampler -- and four tables of u = (x - center) * scale come out:

    moment      [p, p]   sum over all draws of u u^T            chain_sums  [C, p]   per chain, sum over time of u
    chain_outer [p, p]   sum over chains of S_c S_c^T           sum         [p]      sum over chains of S_c

    beta, info = find_map(model)                                       # centre and scale: the mode and the Laplace sd ...
    center, scale = covariance_scaling(beta, info["sd"])               # ... or mean and sd of a short summary_only pilot run
    acc = Covariance(chains=4096, p=8, dtype="float32", center=center, scale=scale)
    res = mcmc(init, kern, iters=1000, summary_only=True, covariance=acc)["covariance"]   # no sample matrix anywhere
    res["cor"], res["rhat_mv"], metric(res)["dmm"]

Because the chains stay apart in `chain_sums`, the same tables give the within-chain and the between-chain covariance matrices W and B
and the multivariate potential scale reduction factor of Brooks & Gelman (1998).  The tables are the same bytes however the draws are
cut into calls.  There is no CPU path: without a GPU the first `update` raises `LogregHipError` like everything else in this package.
`result_from_tables`, `metric`, `covariance_scaling` and `merge_covariance` are pure NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._accum import BlockAccumulator
from ._lib import COV_MAX_P, check

TABLES = ("moment", "chain_outer", "sum", "chain_sums")


def covariance_scaling(center, sd):
    """(center, 1 / sd) in float64, per coordinate: what `Covariance` takes as `center` and `scale`.  The same two sources as
    `marginal_grid`: `find_map`'s mode and its `info["sd"]`, or the `mean` and `sd` of a short `mcmc(..., summary_only=True)` pilot
    run.  They only have to be roughly right: u = (x - center) / sd of about 1 keeps every digit in M - s s^T / N."""
    center, sd = np.asarray(center, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    if center.shape != sd.shape or center.ndim != 1:
        raise ValueError(f"center and sd must be vectors of one length; got {center.shape}, {sd.shape}")
    with np.errstate(divide="ignore", over="ignore"):
        scale = 1.0 / sd
    if not (np.all(np.isfinite(center)) and np.all(np.isfinite(sd)) and np.all(sd > 0) and np.all(np.isfinite(scale))):
        raise ValueError("center must be finite, sd finite and positive")
    return center.copy(), scale


def _scaling(center, scale, p):
    if center is None or scale is None:
        raise ValueError("center and scale (one pair per coordinate; see covariance_scaling) are required")
    center, scale = np.array(center, dtype=np.float64, ndmin=1), np.array(scale, dtype=np.float64, ndmin=1)
    if center.shape != (p,) or scale.shape != (p,):
        raise ValueError(f"center and scale must have length p={p}; got {center.shape}, {scale.shape}")
    if not (np.all(np.isfinite(center)) and np.all(np.isfinite(scale)) and np.all(scale > 0)):
        raise ValueError("center must be finite, scale finite and positive")
    return center, scale


def _lambda_max(W, Bn):
    """largest eigenvalue of W^-1 Bn for symmetric W, Bn; NaN unless both are finite and W is positive definite beyond rounding (a
    pivot of its Cholesky factor below p eps times the largest diagonal entry counts as zero)"""
    if not (np.all(np.isfinite(W)) and np.all(np.isfinite(Bn))):
        return np.nan
    try:
        L = np.linalg.cholesky(W)
        if np.min(np.diag(L)) ** 2 <= W.shape[0] * np.finfo(np.float64).eps * np.max(np.diag(W)):
            return np.nan
        A = np.linalg.solve(L, np.linalg.solve(L, Bn).T)  # L^-1 Bn L^-T, symmetric
        lam = float(np.linalg.eigvalsh((A + A.T) / 2.0)[-1])
    except np.linalg.LinAlgError:
        return np.nan
    return lam if np.isfinite(lam) else np.nan


def result_from_tables(moment, chain_outer, sum, chain_sums, n_draws: int, center, scale) -> dict:
    """The result dict from the four tables of `chains = chain_sums.shape[0]` chains of `n_draws` draws each.  With N = n C, m = s / N
    (the mean of u) and D = diag(1 / scale):

        mean     center + D m                                  cov      D (M - s s^T / N) D / (N - 1)      (np.cov of the pooled draws)
        sd       sqrt(diag(cov))                               cor      cov_ij / (sd_i sd_j); NaN where a variance is <= 0
        within   W = D (M - Q / n) D / (C (n - 1))             between  B = n D (Q / n^2 - C m m^T) D / (C - 1)
        rhat     sqrt(((n - 1) / n W_jj + B_jj / n) / W_jj)    per coordinate, from the diagonals, UNSPLIT: every chain is one sequence
                 (`mcmc(summary_only=True)["rhat"]` is the split figure: each chain cut into batches)
        rhat_mv  (n - 1) / n + (C + 1) / C lambda_max(W^-1 B / n)   Brooks & Gelman (1998); NaN when C < 2, n < 2 or W is singular
        mcse_chains  sqrt(B_jj / (n C)): the standard error of `mean` from the spread of the chain means

    and nobs = N, chains, n_draws, center, scale and the four tables (what `merge_covariance` takes)."""
    M = np.array(moment, dtype=np.float64)
    Q = np.array(chain_outer, dtype=np.float64)
    s = np.array(sum, dtype=np.float64)
    S = np.array(chain_sums, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or Q.shape != M.shape or s.shape != (M.shape[0],) or S.ndim != 2 or S.shape[1] != M.shape[0] or S.shape[0] < 1:
        raise ValueError(f"moment and chain_outer must be [p, p], sum [p] and chain_sums [C, p]; got {M.shape}, {Q.shape}, {s.shape}, {S.shape}")
    p, Cn, n = M.shape[0], S.shape[0], int(n_draws)
    center, scale = _scaling(center, scale, p)
    if n < 0:
        raise ValueError(f"n_draws must not be negative; got {n_draws}")
    N = n * Cn
    d = 1.0 / scale
    DD = np.outer(d, d)
    nan_v, nan_m = np.full(p, np.nan), np.full((p, p), np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = s / N if N else nan_v
        A = M - np.outer(s, s) / N if N else nan_m  # sum of (u - m)(u - m)^T over all draws
        mean = center + d * m
        cov = A * DD / (N - 1.0) if N > 1 else nan_m
        var = np.diag(cov).copy()
        sd = np.sqrt(np.where(var >= 0, var, np.nan))
        a = np.diag(A).copy()
        ok = np.isfinite(a) & (a > 0) & (N > 1)
        root = np.sqrt(np.where(ok, a, np.nan))
        cor = A / np.outer(root, root)
        cor[np.diag_indices(p)] = np.where(ok, 1.0, np.nan)
        Wu = (M - Q / n) / (Cn * (n - 1.0)) if n > 1 else nan_m
        Bu = n * (Q / (float(n) * n) - Cn * np.outer(m, m)) / (Cn - 1.0) if Cn > 1 and n > 0 else nan_m
        within, between = Wu * DD, Bu * DD
        w, b = np.diag(Wu), np.diag(Bu)
        rhat = np.sqrt(((n - 1.0) / n * w + b / n) / w) if n > 1 else nan_v
        mcse = np.sqrt(np.where(b >= 0, b, np.nan) / (float(n) * Cn)) * d if n > 0 else nan_v
        rhat_mv = np.nan
        if Cn >= 2 and n >= 2 and Cn * (n - 1) >= p:  # (fewer within-chain degrees of freedom than coordinates: W is singular)
            lam = _lambda_max(Wu, Bu / n)
            rhat_mv = (n - 1.0) / n + (Cn + 1.0) / Cn * lam
    return {"nobs": N, "chains": Cn, "n_draws": n, "mean": mean, "cov": cov, "sd": sd, "cor": cor, "within": within, "between": between,
            "rhat": rhat, "rhat_mv": float(rhat_mv), "mcse_chains": mcse, "center": center, "scale": scale,
            "moment": M, "chain_outer": Q, "sum": s, "chain_sums": S}


def metric(res) -> dict:
    """A diagonal metric from a result, in the samplers' own conventions: `{"dmm": 1 / diag(cov), "pre": diag(cov)}` -- `dmm` is the
    diagonal mass matrix `hmcKernel` and `nutsKernel` take (the reference's `dmm=1/pre`), `pre` the diagonal preconditioner of
    `malaKernel` and `ulKernel`.  Every variance must be finite and positive."""
    var = np.diag(np.asarray(res["cov"], dtype=np.float64)).copy()
    if not (np.all(np.isfinite(var)) and np.all(var > 0)):
        raise ValueError("metric needs a finite, positive variance in every coordinate")
    return {"dmm": 1.0 / var, "pre": var}


def dense_metric(res) -> np.ndarray:
    """The dense inverse metric `[p, p]` of `nutsKernel(..., inv_metric=)` from a result: the covariance regularised as the warm-up
    regularises a window's (include/logreg_hip_dense.h), n / (n + 5) cov + 1e-3 * 5 / (n + 5) I with n = nobs the draws behind it.
    (`metric(res)` keeps its two diagonal keys.)  Every variance must be finite and positive."""
    cov = np.asarray(res["cov"], dtype=np.float64)
    var = np.diag(cov)
    if not (np.all(np.isfinite(cov)) and np.all(var > 0)):
        raise ValueError("dense_metric needs a finite covariance with a positive variance in every coordinate")
    n = float(res["nobs"])
    return (n / (n + 5.0)) * (0.5 * (cov + cov.T)) + 1e-3 * (5.0 / (n + 5.0)) * np.eye(cov.shape[0])


def merge_covariance(results, center=None, scale=None) -> dict:
    """Results (or raw `(moment, chain_outer, sum, chain_sums, n)` tuples of `Covariance.tables()`, with `center=` and `scale=`) of
    disjoint sets of chains (shards, ranks) of one run with equal n, center and scale -> the result of the union: moment, chain_outer
    and sum add, the chain sums are concatenated in the order given.  Pure NumPy."""
    items = []
    for r in results:
        if isinstance(r, dict):
            items.append((tuple(r[k] for k in TABLES), int(r["n_draws"]), r["center"], r["scale"]))
        else:
            if center is None or scale is None:
                raise ValueError("merge_covariance: raw tables need center= and scale=")
            items.append((tuple(r[:4]), int(r[4]), center, scale))
    if not items:
        raise ValueError("merge_covariance needs at least one result")
    (M, Q, s, S), n, c0, s0 = items[0]
    c0, s0 = np.asarray(c0, dtype=np.float64), np.asarray(s0, dtype=np.float64)
    M, Q, s, parts = np.array(M, dtype=np.float64), np.array(Q, dtype=np.float64), np.array(s, dtype=np.float64), [np.asarray(S, dtype=np.float64)]
    for (M2, Q2, s2, S2), n2, c2, sc2 in items[1:]:
        if n2 != n or np.shape(M2) != M.shape:
            raise ValueError("merge_covariance: every result must have the same n and p")
        if not (np.array_equal(c2, c0) and np.array_equal(sc2, s0)):
            raise ValueError("merge_covariance: every result must have the same center and scale")
        M, Q, s = M + M2, Q + Q2, s + s2
        parts.append(np.asarray(S2, dtype=np.float64))
    return result_from_tables(M, Q, s, np.concatenate(parts, axis=0), n, c0, s0)


class Covariance(BlockAccumulator):
    """Streaming accumulator of the second cross-moment and the per-chain sums of u = (x - center) * scale of `chains` x `p` series of
    `dtype` draws on `device` (p <= 128).  The device state (the cells of the moment, at most 66 MB, and 8 bytes per series) is
    allocated at the first `update`."""
    _prefix, _bind, _keyword = "lr_cov", "bind_covariance", "covariance"
    _entry_points = "covariance entry points (include/logreg_hip_cov.h)"

    def __init__(self, chains: int, p: int, dtype="float32", center=None, scale=None, device: int = 0):
        super().__init__(chains, p, dtype, device)
        if self.p > COV_MAX_P:
            raise ValueError(f"p must be in 1..{COV_MAX_P}; got {p}")
        self.center, self.scale = _scaling(center, scale, self.p)

    def _create(self, L, out):
        return L.lr_cov_create(self.device, self.lr_dtype, self.chains, self.p, self.center.ctypes.data, self.scale.ctypes.data, out)

    def tables(self):
        """(moment `[p, p]`, chain_outer `[p, p]`, sum `[p]`, chain_sums `[C, p]`, n): float64, NaN before the first draw."""
        h = self.handle
        M, Q = np.empty((self.p, self.p)), np.empty((self.p, self.p))
        s, S = np.empty(self.p), np.empty((self.chains, self.p))
        n = C.c_int64()
        check(self._L.lr_cov_result(h, M.ctypes.data, Q.ctypes.data, s.ctypes.data, S.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return M, Q, s, S, self.n_draws

    def result(self) -> dict:
        """mean, sd, rhat, mcse_chains [p], cov, cor, within, between [p, p], rhat_mv, nobs, chains, n_draws, and the raw tables with
        center and scale: see `result_from_tables`."""
        M, Q, s, S, n = self.tables()
        return result_from_tables(M, Q, s, S, n, self.center, self.scale)

    def __repr__(self):
        return f"Covariance(chains={self.chains}, p={self.p}, dtype={self.dtype.name}, n_draws={self.n_draws})"
