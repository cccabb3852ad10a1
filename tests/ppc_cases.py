"""The cases tests/test_gpu_ppc.py runs and tests/test_ppc_cpu.py checks the undecided share of, with their references computed once per
process.  TEST INFRASTRUCTURE ONLY.

(r, p, S): every width class of the kernel (3 -> 4 padded, 8 unpadded, 17 -> 32, 33 -> 64 rows in registers at float32 and re-read at
float64, 128 re-read in both) and rows of one lane, less than a wave, a tile and a row, and three tiles less 167 rows; r = 1 takes S
up so that the case keeps MIN_PAIRS pairs.  S is never a multiple of 4 plus the first index (FIRST = 5), so the first and the last quad
are partial.
"""
import functools

import numpy as np

import ppc_reference as ppr

FIRST = 5  # the draw index the terms of a case start at: s mod 4 != 0
SEED = 0x9E3779B97F4A7C15
CASES = ((1, 3, 4003), (63, 128, 65), (257, 8, 65), (257, 17, 17), (601, 33, 65))
DTYPES = ("float32", "float64")
GROUPS = (1, 2, 7, 32)


def data(r, p, S, seed=0):
    """X [r, p] (an intercept and normal columns), y [r] drawn from the model at beta0, draws B [S, p] around beta0 with logits of a
    few units: pi spreads over (0, 1)"""
    rng = np.random.default_rng(1000 * r + 10 * p + seed)
    X = np.concatenate([np.ones((r, 1)), rng.standard_normal((r, p - 1))], axis=1)
    beta0 = rng.standard_normal(p) * 1.5 / np.sqrt(p)
    y = (rng.random(r) < 1 / (1 + np.exp(-X @ beta0))).astype(np.float64)
    B = beta0 + 0.3 / np.sqrt(p) * rng.standard_normal((S, p))
    return X, y, B


def groups_for(r, G):
    """labels interleaved across the tiles (i mod (G - 1) or so) with the LAST group empty where G > 1 and the rows allow"""
    if G == 1:
        return None
    return (np.arange(r) * 7 % max(G - 1, 1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(r, p, S, dtype):
    """-> dict: X, y, B, pv (ppc_reference.pair_values), rep, undecided, u at draw indices FIRST .. FIRST + S - 1 with SEED"""
    X, y, B = data(r, p, S)
    pv = ppr.pair_values(X, B, dtype)
    rep, und, u = ppr.replicate(pv, SEED, FIRST)
    return dict(X=X, y=y, B=B, pv=pv, rep=rep, undecided=und, u=u)
