"""A reference of the posterior predictive check of include/logreg_hip_ppc.h -- the replicate of every (draw, row) pair, the per-draw
counts and deviances, the accumulated tables -- with the error bounds of a device path computing in `dtype`.  TEST INFRASTRUCTURE ONLY
(tests/test_ppc_cpu.py checks this file without a GPU; tests/test_gpu_ppc.py holds the kernels to it).

Philox and the 24-bit uniform are those of tests/pg_reference.py; the exact pair values pi, l_1 = log sigma(eta), l_0 = log sigma(-eta) and
their bounds those of tests/pair_reference.py (`pairs` with every label 1, then with every label 0: `l` is then l_1, then l_0).

Undecided pairs.  The device's pi is not the reference's to the last bit, so the replicate [u < pi] is compared only where the uniform
is clear of the reference's pi: a pair is UNDECIDED where |u - pi_ref| <= tol_pi (pair_reference.pair_bounds) and is left out of the
exact comparison.  `UNDECIDED_CAP`: at most 0.1 % of a case's pairs may be undecided, and every case has at least `MIN_PAIRS` pairs.

Deviances.  D = -2 sum_i l: held within  2 sum_i tol_l(i)  +  2 (r + 8) 2^-53 sum_i |l_i|  (the float64 sum of r terms, whatever its
tree), the pair bound of the label each row's term was taken for.  No factor multiplies a bound.
"""
import numpy as np

import pair_reference as pr
import pg_reference as pg

TAG = 0x04000000  # LR_PPC_TAG
UNDECIDED_CAP = 1e-3
MIN_PAIRS = 4000


def uniforms(seed, first_index, S, r, dtype="float64"):
    """u [S, r] as `dtype` forms it, returned as float64 (float32 rounds (w >> 8) + 0.5, 25 bits, to even): word s & 3 of the block with key = seed, counter = (q lo, q hi, i, TAG), q = s >> 2"""
    s = np.arange(first_index, first_index + S, dtype=np.uint64)
    q = s >> np.uint64(2)
    w = pg.philox((q & np.uint64(0xFFFFFFFF))[:, None], (q >> np.uint64(32))[:, None], np.arange(r, dtype=np.uint64)[None, :], TAG, seed, int(seed) >> 32)
    pick = (s & np.uint64(3))[:, None]
    word = np.where(pick == 0, w[0], np.where(pick == 1, w[1], np.where(pick == 2, w[2], w[3])))
    return pg._u(word, np.float32 if dtype == "float32" else np.float64).astype(np.float64)


def pair_values(X, B, dtype):
    """pi, l1, l0 [S, r] float64 with their bounds tol_pi, tol_l1, tol_l0 as a model of `dtype` computes them"""
    r = np.shape(X)[0]
    one, zero = pr.pairs(X, np.ones(r), B, dtype), pr.pairs(X, np.zeros(r), B, dtype)
    b1, b0 = pr.pair_bounds(one), pr.pair_bounds(zero)
    return dict(dtype=dtype, pi=one["pi"], l1=one["l"], l0=zero["l"], tol_pi=b1["pi"], tol_l1=b1["l"], tol_l0=b0["l"])


def replicate(pv, seed, first_index=0):
    """-> rep [S, r] bool (the reference's replicate), undecided [S, r] bool, u"""
    S, r = pv["pi"].shape
    u = uniforms(seed, first_index, S, r, pv["dtype"])
    return u < pv["pi"], np.abs(u - pv["pi"]) <= pv["tol_pi"], u


def unpack(bits, r):
    """bits [S, ceil(r / 32)] uint32 -> [S, r] bool"""
    bits = np.asarray(bits, dtype=np.uint32)
    i = np.arange(r)
    return ((bits[:, i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def counts_of(rep, groups, G):
    """T_g per draw: [S, G] int64 from rep [S, r] bool"""
    groups = np.zeros(rep.shape[1], dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    return np.stack([rep[:, groups == g].sum(axis=1) for g in range(G)], axis=1).astype(np.int64)


def deviance(pv, labels):
    """D [S] = -2 sum_i l_{labels} and its bound, labels [r] or [S, r] in {0, 1} (bool); longdouble sums"""
    lab = np.broadcast_to(np.asarray(labels, dtype=bool), pv["pi"].shape)
    l = np.where(lab, pv["l1"], pv["l0"]).astype(np.longdouble)
    tol = np.where(lab, pv["tol_l1"], pv["tol_l0"]).astype(np.longdouble)
    r = l.shape[1]
    D = -2 * l.sum(axis=1)
    bound = 2 * tol.sum(axis=1) + 2 * (r + 8) * np.longdouble(2.0 ** -53) * np.abs(l).sum(axis=1)
    return D.astype(np.float64), bound.astype(np.float64)


def accumulate(counts, dev, rep, n_g, finite=None):
    """The tables of the header from per-draw quantities (counts [S, G], dev [S, 2], rep [S, r] bool): a host recount.
    -> dict hist [r + G] uint64, row_ones [r] uint64, counts [2] uint64, moments [4] (two-pass, longdouble), n_draws"""
    counts, dev = np.asarray(counts, dtype=np.int64), np.asarray(dev, dtype=np.float64)
    S, G = counts.shape
    fin = np.ones(S, dtype=bool) if finite is None else np.asarray(finite, dtype=bool)
    n_g = np.asarray(n_g, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n_g + 1)])
    hist = np.zeros(int(off[-1]), dtype=np.uint64)
    for g in range(G):
        hist[off[g]:off[g + 1]] = np.bincount(counts[fin, g], minlength=int(n_g[g]) + 1).astype(np.uint64)
    mom = np.full(4, np.nan)
    if fin.any():
        for k in range(2):
            v = dev[fin, k].astype(np.longdouble)
            m = v.sum() / np.longdouble(v.size)
            mom[2 * k], mom[2 * k + 1] = float(m), float(((v - m) ** 2).sum())
    with np.errstate(invalid="ignore"):
        ge = int(np.sum(dev[fin, 1] >= dev[fin, 0]))
    return dict(hist=hist, row_ones=rep[fin].sum(axis=0).astype(np.uint64), counts=np.array([ge, int((~fin).sum())], dtype=np.uint64), moments=mom, n_draws=S)


def moment_bounds(dev, dev_bound=None):
    """[4] tolerances of the moment rows against `accumulate` of the same per-draw values: pair_reference.table_bounds' accumulation
    term, (S + 8) 2^-53 (M2 + S max (v - m)^2) + floor64 for an M2; for a mean (S + 8) 2^-53 max |v|."""
    dev = np.asarray(dev, dtype=np.float64)
    S = dev.shape[0]
    out = np.empty(4)
    for k in range(2):
        v = dev[:, k].astype(np.longdouble)
        m = v.sum() / np.longdouble(S)
        d = np.abs(v - m)
        out[2 * k] = float((S + 8) * np.longdouble(2.0 ** -53) * np.abs(v).max())
        out[2 * k + 1] = float((S + 8) * np.longdouble(2.0 ** -53) * ((d * d).sum() + S * d.max() ** 2)) + pr.FLOOR64
    return out
