"""Autocorrelation and Geyer's effective sample size of the kept draws, on the device.

`diagnostics.ess_geyer` is the estimator the project's ESS figures are stated in, but it is a host loop over chains on the whole
`[iters, C, p]` matrix.  `Autocorr` is the same estimator, restricted to the first `max_lag` lags, as a streaming accumulator that
takes the draws where they are (include/logreg_hip_acf.h, kernels in csrc/lr_acf.h): blocks `[k, C, p]` in time order go in -- NumPy
arrays or the `DeviceArray` blocks `ChainSet.advance` returns, from any sampler -- and a table of chain-pooled sums comes out:

    row 0        sum over chains of the per-chain ESS        (= diagnostics.ess_pooled(samples, max_chains=None) where no series is capped)
    row 1        number of capped chains (no Gamma_j <= 0 within (max_lag + 1) / 2 pairs, though the series is long enough for more)
    row 2        number of chains whose ESS is NaN (a NaN or an inf among their draws)
    row 3 + l    sum over chains of the autocovariance at lag l, l = 0 .. max_lag

    ac = Autocorr(chains=4096, p=8, dtype="float32")
    res = mcmc(init, kern, iters=1000, summary_only=True, autocorr=ac)     # no sample matrix anywhere
    res["autocorr"]["ess"], res["autocorr"]["acf"][:11]

There is no CPU path: without a GPU the first `update` raises `LogregHipError` like everything else in this package.
`merge_autocorr` (pure NumPy) combines the results of chain shards: every row is a sum over chains, so the tables add.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._accum import BlockAccumulator
from ._lib import ACF_HEAD_ROWS, ACF_MAX_LAG, check


def geyer_tau(rho, n: int) -> float:
    """tau = -1 + 2 sum of Gamma_j = rho[2j] + rho[2j+1] over j < min(len(rho) // 2, n // 2), truncated at the first Gamma_j <= 0: the
    scan of `diagnostics.ess_geyer` on an autocorrelation sequence that is already there."""
    rho = np.asarray(rho, dtype=np.float64)
    pairs = min(rho.shape[0] // 2, int(n) // 2)
    gam = rho[0:2 * pairs:2] + rho[1:2 * pairs:2]
    nonpos = np.nonzero(~(gam > 0.0))[0]
    k = int(nonpos[0]) if nonpos.size else pairs
    return -1.0 + 2.0 * float(np.sum(gam[:k]))


def result_from_sums(sums, ess_chain, n: int, chains: int) -> dict:
    """The result dict from a table `[max_lag + 4, p]` of `chains` chains of `n` draws each (and their per-chain ESS `[chains, p]`)."""
    S = np.asarray(sums, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] < ACF_HEAD_ROWS + 2 or (S.shape[0] - ACF_HEAD_ROWS) % 2:
        raise ValueError(f"sums must be [max_lag + 4, p] with max_lag odd; got {S.shape}")
    K, p = S.shape[0] - ACF_HEAD_ROWS - 1, S.shape[1]
    n, Cn = int(n), int(chains)
    acov = S[ACF_HEAD_ROWS:]
    with np.errstate(divide="ignore", invalid="ignore"):
        acf = acov / acov[0]
        ess_acf = np.full(p, np.nan)
        for j in range(p):
            if not np.all(np.isfinite(acf[:, j])) and not (n < 4 and np.isfinite(acov[0, j])):
                continue  # a non-finite series among the chains (or no variance at all): NaN
            tau = geyer_tau(acf[:, j], n) if n >= 4 else 1.0
            ess_acf[j] = Cn * n / tau if tau > 0.0 else float(Cn * n)
        mcse = np.sqrt(acov[0] / Cn / S[0]) if n > 0 else np.full(p, np.nan)
    return {"n": n, "chains": Cn, "max_lag": K, "ess": S[0].copy(), "ess_chain": np.asarray(ess_chain, dtype=np.float64),
            "capped": S[1].copy(), "nan_chains": S[2].copy(), "acf": acf, "ess_pooled_acf": ess_acf, "mcse": mcse, "sums": S.copy()}


def merge_autocorr(results) -> dict:
    """Results of disjoint sets of chains (shards, ranks) of one run -> the result of the union: the sums add, the per-chain ESS are
    concatenated in the order given.  Pure NumPy."""
    results = list(results)
    if not results:
        raise ValueError("merge_autocorr needs at least one result")
    n, K, shape = results[0]["n"], results[0]["max_lag"], results[0]["sums"].shape
    if any(r["n"] != n or r["max_lag"] != K or r["sums"].shape != shape for r in results):
        raise ValueError("merge_autocorr: every result must have the same n, max_lag and p")
    sums = np.zeros(shape)
    for r in results:
        sums = sums + r["sums"]
    return result_from_sums(sums, np.concatenate([r["ess_chain"] for r in results], axis=0), n, sum(r["chains"] for r in results))


class Autocorr(BlockAccumulator):
    """Streaming accumulator of the lag-0..max_lag autocovariance and Geyer ESS of `chains` x `p` series of `dtype` draws on `device`.
    The device state (about 8 (3 max_lag + 3) bytes per series) is allocated at the first `update`."""
    _prefix, _bind, _keyword = "lr_acf", "bind_acf", "autocorr"
    _entry_points = "autocorrelation entry points (include/logreg_hip_acf.h)"

    def __init__(self, chains: int, p: int, dtype="float32", max_lag: int = 63, device: int = 0):
        super().__init__(chains, p, dtype, device, max_lag=max_lag)
        if not 1 <= self.max_lag <= ACF_MAX_LAG or self.max_lag % 2 == 0:
            raise ValueError(f"max_lag must be odd and in 1..{ACF_MAX_LAG} (lags 0..max_lag are (max_lag + 1) / 2 Geyer pairs); got {max_lag}")

    def _create(self, L, out):
        return L.lr_acf_create(self.device, self.lr_dtype, self.chains, self.p, self.max_lag, out)

    def sums(self):
        """(table `[max_lag + 4, p]`, per-chain ESS `[C, p]`), float64; NaN everywhere before the first draw."""
        h = self.handle
        out = np.empty((self.max_lag + 1 + ACF_HEAD_ROWS, self.p), dtype=np.float64)
        ess = np.empty((self.chains, self.p), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_acf_result(h, out.ctypes.data, ess.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return out, ess

    def result(self) -> dict:
        """n, chains, max_lag, ess [p] (sum of the per-chain Geyer ESS), ess_chain [C, p], capped [p], nan_chains [p], acf [max_lag + 1, p]
        (the pooled autocorrelation: sum_c acov_c[l] / sum_c acov_c[0]), ess_pooled_acf [p] (C n / tau of the Geyer scan on that pooled
        autocorrelation: the stable figure when chains are many and short), mcse [p] (sqrt(mean_c acov_c[0] / ess)), sums (the table)."""
        sums, ess = self.sums()
        return result_from_sums(sums, ess, self.n_draws, self.chains)

    def __repr__(self):
        return f"Autocorr(chains={self.chains}, p={self.p}, dtype={self.dtype.name}, max_lag={self.max_lag}, n_draws={self.n_draws})"
