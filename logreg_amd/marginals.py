"""Marginal histograms, quantiles and higher moments of the kept draws, on the device.

What the reference prints last -- `scipy.stats.describe(out)` (nobs, min/max, mean, variance, skewness, kurtosis) and the quartiles and
histograms of `smfsb::mcmcSummary` -- needs the whole `[iters, C, p]` matrix on the host.  `Marginals` is the streaming accumulator for
it (include/logreg_hip_marginals.h, kernels in csrc/lr_marginals.h): blocks `[k, C, p]` in time order go in -- NumPy arrays or the
`DeviceArray` blocks `ChainSet.advance` returns, from any sampler -- and two tables, pooled over chains and time, come out:

    counts [p, bins + 3] uint64     column 0 underflow (x < lo), 1 .. bins the grid, bins + 1 overflow (x >= hi), bins + 2 NaN
    table  [6, p] float64           min, max over the non-NaN draws; S1..S4 = sum u^k of u = (x - (lo + hi) / 2) * 2 / (hi - lo)

    beta, info = find_map(model)                                       # the grid: mode -+ 8 sd of the Laplace approximation ...
    lo, hi = marginal_grid(beta, info["sd"])                           # ... or mean -+ 8 sd of a short summary_only pilot run
    mg = Marginals(chains=4096, p=8, dtype="float32", lo=lo, hi=hi)
    res = mcmc(init, kern, iters=1000, summary_only=True, marginals=mg)["marginals"]      # no sample matrix anywhere
    res["skewness"], quantile(res, [0.025, 0.5, 0.975]), hpd(res, 0.9)

The counts are exact integers; the sums are the same bytes however the draws are cut into calls.  Quantiles are read off the
histogram: the estimate and the exact order statistic lie in the same column, so inside the grid the error is at most one bin width,
(hi - lo) / bins.  There is no CPU path: without a GPU the first `update` raises `LogregHipError` like everything else in this package.
`result_from_tables`, `quantile`, `interval`, `hpd` and `merge_marginals` are pure NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._accum import BlockAccumulator
from ._lib import MARG_MAX_BINS, MARG_ROWS, check


def marginal_grid(center, scale, width: float = 8.0):
    """(lo, hi) = center -+ width * scale, per coordinate.  Two sources of centre and scale: `find_map`'s mode and its `info["sd"]` (the
    Laplace approximation about the mode), or the `mean` and `sd` of a short `mcmc(..., summary_only=True)` pilot run.  Draws outside
    the grid are not lost: they land in the underflow / overflow columns and still count in min / max and the moments."""
    center, scale = np.asarray(center, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    if center.shape != scale.shape or center.ndim != 1:
        raise ValueError(f"center and scale must be vectors of one length; got {center.shape}, {scale.shape}")
    if not (np.all(np.isfinite(center)) and np.all(np.isfinite(scale)) and np.all(scale > 0) and np.isfinite(width) and width > 0):
        raise ValueError("center must be finite, scale and width finite and positive")
    return center - width * scale, center + width * scale


def _grid(lo, hi, p):
    lo, hi = np.array(lo, dtype=np.float64, ndmin=1), np.array(hi, dtype=np.float64, ndmin=1)
    if lo.shape != (p,) or hi.shape != (p,):
        raise ValueError(f"lo and hi must have length p={p}; got {lo.shape}, {hi.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        ok = np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi) and np.all(np.isfinite(hi - lo))
    if not ok:
        raise ValueError("lo and hi must be finite with lo < hi in every coordinate")
    return lo, hi


def result_from_tables(counts, table, lo, hi, n_draws: int, chains: int) -> dict:
    """The result dict from the tables `counts [p, bins + 3]` and `table [6, p]` of `chains` chains of `n_draws` draws each on the grid
    `lo`, `hi`.  Moments as `scipy.stats.describe` defines them: variance with ddof = 1, skewness m3 / m2^1.5 and kurtosis
    m4 / m2^2 - 3 from the biased central moments (bias=True)."""
    cnt = np.asarray(counts)
    tab = np.asarray(table, dtype=np.float64)
    if cnt.ndim != 2 or cnt.shape[1] < 4 or tab.shape != (MARG_ROWS, cnt.shape[0]) or cnt.dtype.kind not in "iu":
        raise ValueError(f"counts must be integers [p, bins + 3] and table [6, p]; got {cnt.shape} {cnt.dtype}, {tab.shape}")
    cnt = cnt.astype(np.uint64)
    p, B = cnt.shape[0], cnt.shape[1] - 3
    lo, hi = _grid(lo, hi, p)
    n, Cn = int(n_draws), int(chains)
    nobs = n * Cn
    half = (hi - lo) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        N = float(nobs) if nobs else np.nan
        a1, a2, a3, a4 = tab[2] / N, tab[3] / N, tab[4] / N, tab[5] / N  # raw moments of u
        m2 = a2 - a1 * a1
        m3 = a3 - 3.0 * a1 * a2 + 2.0 * a1 ** 3
        m4 = a4 - 4.0 * a1 * a3 + 6.0 * a1 * a1 * a2 - 3.0 * a1 ** 4
        mean = (lo + hi) / 2.0 + a1 * half
        variance = m2 * half * half * (nobs / (nobs - 1.0)) if nobs > 1 else np.full(p, np.nan)
        skewness = m3 / m2 ** 1.5
        kurtosis = m4 / (m2 * m2) - 3.0
        inside = cnt[:, 1:B + 1]
        valid = nobs - cnt[:, B + 2].astype(np.float64)
        width = (hi - lo) / B
        density = inside / (valid * width)[:, None]
    edges = lo[:, None] + (hi - lo)[:, None] * (np.arange(B + 1) / B)[None, :]
    edges[:, B] = hi
    return {"nobs": nobs, "n": n, "chains": Cn, "bins": B, "lo": lo, "hi": hi, "minmax": (tab[0].copy(), tab[1].copy()), "mean": mean,
            "variance": variance, "skewness": skewness, "kurtosis": kurtosis, "counts": inside.copy(), "edges": edges, "density": density,
            "underflow": cnt[:, 0].copy(), "overflow": cnt[:, B + 1].copy(), "nan": cnt[:, B + 2].copy(), "columns": cnt, "table": tab.copy()}


def _column_edges(res, j):
    """left and right end of the bins + 2 value columns of coordinate j: underflow = [min, lo], overflow = [hi, max]"""
    B = res["bins"]
    left = np.empty(B + 2)
    right = np.empty(B + 2)
    left[1:B + 1], right[1:B + 1] = res["edges"][j, :B], res["edges"][j, 1:]
    left[0], right[0] = res["minmax"][0][j], res["lo"][j]
    left[B + 1], right[B + 1] = res["hi"][j], res["minmax"][1][j]
    return left, right


def quantile(res, q):
    """The q-quantile(s) of every coordinate from its histogram -> [len(q), p] (or [p] for a scalar q).  N = the coordinate's non-NaN
    draws, r = max(1, ceil(q N)): the column whose cumulative count first reaches r holds the r-th smallest draw (the quantile
    `np.quantile(..., method="inverted_cdf")` returns); inside it the estimate is interpolated linearly in rank (the i-th of the
    column's k draws at (i - 1/2) / k of its width, and never beyond the smallest or the largest draw).  The underflow column spans
    [min, lo] and the overflow column [hi, max], so a finite sample always gets a finite answer; a coordinate without a non-NaN draw gets
    NaN."""
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or not np.all((qs >= 0) & (qs <= 1)):
        raise ValueError("q must be in [0, 1]")
    B, p = res["bins"], res["columns"].shape[0]
    out = np.full((qs.size, p), np.nan)
    for j in range(p):
        col = res["columns"][j, :B + 2].astype(np.int64)
        cum = np.cumsum(col)
        N = int(cum[-1])
        if N == 0:
            continue
        left, right = _column_edges(res, j)
        for i, qq in enumerate(qs):
            r = max(1, int(np.ceil(qq * N)))
            c = int(np.searchsorted(cum, r, side="left"))
            before = int(cum[c - 1]) if c else 0
            frac = (r - before - 0.5) / int(col[c])
            a, b = left[c], right[c]
            est = a if np.isinf(a) else b if np.isinf(b) else a + (b - a) * frac
            out[i, j] = min(max(est, left[0]), right[B + 1])  # (never beyond the smallest and the largest draw)
    return out if np.ndim(q) else out[0]


def interval(res, level: float = 0.95):
    """The equal-tailed credible interval of every coordinate -> [2, p]: the (1 - level) / 2 and (1 + level) / 2 quantiles."""
    if not 0 < level < 1:
        raise ValueError("level must be in (0, 1)")
    return quantile(res, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])


def hpd(res, level: float = 0.95):
    """The shortest run of consecutive columns that holds at least ceil(level N) of a coordinate's N non-NaN draws -> [2, p]: its left and
    right end (the first such run where several are equally short): the highest-density interval to the resolution of the grid."""
    if not 0 < level < 1:
        raise ValueError("level must be in (0, 1)")
    B, p = res["bins"], res["columns"].shape[0]
    out = np.full((2, p), np.nan)
    for j in range(p):
        col = res["columns"][j, :B + 2].astype(np.int64)
        cum = np.concatenate([[0], np.cumsum(col)])
        N = int(cum[-1])
        if N == 0:
            continue
        need = max(1, int(np.ceil(level * N)))
        left, right = _column_edges(res, j)
        best = None
        for i in range(B + 2):
            if col[i] == 0:
                continue  # (a run never starts on an empty column: the next start is as good and shorter)
            e = int(np.searchsorted(cum, cum[i] + need, side="left")) - 1  # first column at which the run holds `need`
            if e > B + 1:
                break
            w = right[e] - left[i]
            if best is None or w < best[0]:
                best = (w, left[i], right[e])
        out[:, j] = best[1:]
    return out


def merge_marginals(results) -> dict:
    """Results of disjoint sets of chains (shards, ranks) of one run on one grid -> the result of the union: counts and power sums add,
    min and max combine.  Pure NumPy."""
    results = list(results)
    if not results:
        raise ValueError("merge_marginals needs at least one result")
    first = results[0]
    for r in results[1:]:
        if r["n"] != first["n"] or r["bins"] != first["bins"] or r["columns"].shape != first["columns"].shape:
            raise ValueError("merge_marginals: every result must have the same n, bins and p")
        if not (np.array_equal(r["lo"], first["lo"]) and np.array_equal(r["hi"], first["hi"])):
            raise ValueError("merge_marginals: every result must be on the same grid (lo, hi)")
    counts = np.zeros_like(first["columns"])
    table = np.array(first["table"])
    for i, r in enumerate(results):
        counts = counts + r["columns"]
        if i:
            with np.errstate(invalid="ignore"):
                table[0] = np.fmin(table[0], r["table"][0])  # (NaN: that shard has no non-NaN draw of the coordinate)
                table[1] = np.fmax(table[1], r["table"][1])
                table[2:] = table[2:] + r["table"][2:]
    return result_from_tables(counts, table, first["lo"], first["hi"], first["n"], sum(r["chains"] for r in results))


class Marginals(BlockAccumulator):
    """Streaming accumulator of the marginal histograms (`bins` bins on [lo_j, hi_j) per coordinate), min / max and power sums of `chains`
    x `p` series of `dtype` draws on `device`.  The device state (8 p (bins + 3) bytes of counts and 48 bytes per series) is allocated
    at the first `update`."""
    _prefix, _bind, _keyword = "lr_marg", "bind_marginals", "marginals"
    _entry_points = "marginals entry points (include/logreg_hip_marginals.h)"

    def __init__(self, chains: int, p: int, dtype="float32", lo=None, hi=None, bins: int = 256, device: int = 0):
        super().__init__(chains, p, dtype, device, bins=bins)
        if not 1 <= self.bins <= MARG_MAX_BINS:
            raise ValueError(f"bins must be in 1..{MARG_MAX_BINS}; got {bins}")
        if lo is None or hi is None:
            raise ValueError("lo and hi (the grid, one pair per coordinate; see marginal_grid) are required")
        self.lo, self.hi = _grid(lo, hi, self.p)

    def _create(self, L, out):
        return L.lr_marg_create(self.device, self.lr_dtype, self.chains, self.p, self.bins, self.lo.ctypes.data, self.hi.ctypes.data, out)

    def counts_table(self):
        """(counts `[p, bins + 3]` uint64, table `[6, p]` float64); zeros and NaN before the first draw."""
        h = self.handle
        counts = np.empty((self.p, self.bins + 3), dtype=np.uint64)
        table = np.empty((MARG_ROWS, self.p), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_marg_result(h, counts.ctypes.data, table.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return counts, table

    def result(self) -> dict:
        """nobs, minmax, mean, variance, skewness, kurtosis [p] (as scipy.stats.describe's), counts [p, bins], edges [p, bins + 1],
        density [p, bins], underflow, overflow, nan [p], and the raw tables (columns [p, bins + 3], table [6, p]) with the grid: what
        `quantile`, `interval`, `hpd` and `merge_marginals` take."""
        counts, table = self.counts_table()
        return result_from_tables(counts, table, self.lo, self.hi, self.n_draws, self.chains)

    def __repr__(self):
        return f"Marginals(chains={self.chains}, p={self.p}, dtype={self.dtype.name}, bins={self.bins}, n_draws={self.n_draws})"
