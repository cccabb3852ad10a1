"""Rank-normalised split-R-hat with bulk and tail effective sample sizes of the kept draws, on the device.

`diagnostics.split_rhat` is the mean / variance R-hat: blind to chains that differ in scale, meaningless under heavy tails.
`RankDiagnostics` reports what Stan, ArviZ and `posterior` report since Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021) -- R-hat
of the rank-normalised and of the folded draws, bulk-ESS and tail-ESS -- as an accumulator that takes the draws where they are
(include/logreg_hip_rank.h states the definition line by line; kernels in csrc/lr_rank.h).  Ranks need a global order, so unlike the
other accumulators this one stores the blocks `[k, C, p]` it is fed (device memory, `max_steps` steps at the most, chains x max_steps <=
2^24) and sorts them when `result()` is called:

    rk = RankDiagnostics(chains=4096, p=8, max_steps=1000, dtype="float32")
    res = mcmc(init, kern, iters=1000, summary_only=True, rank=rk)        # no sample matrix anywhere
    res["rank"]["rhat"], res["rank"]["ess_bulk"], res["rank"]["ess_tail"]

There is no CPU path: without a GPU the first `update` raises `LogregHipError` like everything else in this package.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._accum import BlockAccumulator
from ._lib import RANK_MAX_DRAWS, RANK_MAX_LAG, RANK_ROWS, check

_FLOAT_ROWS = ("rhat_bulk", "rhat_tail", "rhat", "ess_bulk", "ess_tail", "capped_bulk", "capped_q05", "capped_q95", "median", "q05", "q95")


def rank_result_from_table(table, n: int, chains: int, max_lag: int) -> dict:
    """The result dict from a table `[LR_RANK_ROWS, p]` of `chains` chains of `n` stored steps.  Pure NumPy."""
    T = np.asarray(table, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != RANK_ROWS:
        raise ValueError(f"table must be [{RANK_ROWS}, p]; got {T.shape}")
    res = {name: T[i].copy() for i, name in enumerate(_FLOAT_ROWS)}
    res.update(n_nonfinite=T[11].astype(np.int64), pairs_bulk=T[12].copy(), pairs_q05=T[13].copy(), pairs_q95=T[14].copy(),
               n=int(n), n_used=int(n) // 2 * 2, chains=int(chains), max_lag=int(max_lag), table=T.copy())
    return res


class RankDiagnostics(BlockAccumulator):
    """Accumulator of rank-normalised split-R-hat, bulk-ESS and tail-ESS of `chains` x `p` series of `dtype` draws on `device`, with
    room for `max_steps` time steps (chains x max_steps x p values of `dtype` in device memory, allocated at the first `update`)."""
    _prefix, _bind, _keyword = "lr_rank", "bind_rank", "rank"
    _entry_points = "rank-diagnostics entry points (include/logreg_hip_rank.h)"

    def __init__(self, chains: int, p: int, max_steps: int, dtype="float32", device: int = 0, max_lag: int = 63):
        super().__init__(chains, p, dtype, device, max_steps=max_steps, max_lag=max_lag)
        if self.max_steps <= 0:
            raise ValueError(f"max_steps must be positive; got {max_steps}")
        if not 1 <= self.max_lag <= RANK_MAX_LAG or self.max_lag % 2 == 0:
            raise ValueError(f"max_lag must be odd and in 1..{RANK_MAX_LAG} (lags 0..max_lag are (max_lag + 1) / 2 pairs); got {max_lag}")
        if self.chains * self.max_steps > RANK_MAX_DRAWS:
            raise ValueError(f"chains x max_steps = {self.chains} x {self.max_steps} is beyond the cap of {RANK_MAX_DRAWS} draws per coordinate")

    def _create(self, L, out):
        return L.lr_rank_create(self.device, self.lr_dtype, self.chains, self.p, self.max_steps, self.max_lag, out)

    def check_block(self, shape, dtype=None, device=None):
        super().check_block(shape, dtype, device)
        if self.n_draws + int(shape[0]) > self.max_steps:
            raise ValueError(f"{int(shape[0])} more steps after {self.n_draws} exceed max_steps = {self.max_steps}")

    def check_run(self, chains, model, iters):
        super().check_run(chains, model, iters)
        if self.n_draws + int(iters) > self.max_steps:
            raise ValueError(f"rank= has room for max_steps = {self.max_steps} steps and holds {self.n_draws}; this run keeps {int(iters)} more")

    def table(self):
        """The result table `[LR_RANK_ROWS, p]`, float64 (rows: include/logreg_hip_rank.h)."""
        h = self.handle
        out = np.empty((RANK_ROWS, self.p), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_rank_result(h, out.ctypes.data, C.byref(n)))
        self.n_draws = int(n.value)
        return out

    def result(self) -> dict:
        """Per coordinate `[p]`: rhat_bulk, rhat_tail, rhat (the larger), ess_bulk, ess_tail, capped_bulk / capped_q05 / capped_q95 (the
        lags ran out at max_lag), median, q05, q95 (exact order statistics), n_nonfinite, pairs_bulk / pairs_q05 / pairs_q95 (pairs kept);
        and n, n_used (= 2 (n // 2)), chains, max_lag, table."""
        return rank_result_from_table(self.table(), self.n_draws, self.chains, self.max_lag)

    def ranks(self, j: int, folded: bool = False, with_z: bool = False):
        """Twice the average rank of every used draw of coordinate `j` (`folded`: of |x - median|), int64 `[2 (n // 2), C]` in time order:
        what a rank histogram per chain is drawn from.  `with_z`: -> (ranks, their z-scale as float64)."""
        j = int(j)
        if not 0 <= j < self.p:
            raise ValueError(f"coordinate must be in 0..{self.p - 1}; got {j}")
        h = self.handle
        used = self.n_draws // 2 * 2
        r2 = np.empty((used, self.chains), dtype=np.int64)
        z = np.empty((used, self.chains), dtype=np.float64)
        n = C.c_int64()
        check(self._L.lr_rank_ranks(h, j, int(bool(folded)), r2.ctypes.data, z.ctypes.data, C.byref(n)))
        if int(n.value) != used:
            raise RuntimeError(f"the library holds {n.value} used steps, this object counted {used}")
        return (r2, z) if with_z else r2

    def __repr__(self):
        return (f"RankDiagnostics(chains={self.chains}, p={self.p}, max_steps={self.max_steps}, dtype={self.dtype.name}, max_lag={self.max_lag}, "
                f"n_draws={self.n_draws})")
