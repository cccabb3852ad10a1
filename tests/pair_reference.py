"""A per-pair reference of the posterior-predictive quantities of include/logreg_hip_predict.h -- pi, L and l of every (draw, row)
pair -- that stays exact where |t| = |x . beta| is large, the table of the header built from it, and the error bounds of a device path
computing in `dtype`, stated once and from the inputs alone.  TEST INFRASTRUCTURE ONLY (tests/test_predict_regimes_cpu.py checks this
file without a GPU; tests/test_gpu_predict_regimes.py holds the kernels to it).

    eta = x_i . beta_s     pi = sigma(eta)     t = (2 y_i - 1) eta     L = sigma(t)     l = log sigma(t) = min(t, 0) - log1p(exp(-|t|))

Arithmetic.  The logit is the exact one of tests/eval_reference.py (`logits`: every product split in two doubles, math.fsum taken twice: a
head and a residual).  The pair terms are numpy.longdouble (64-bit significand, exponent range to 1e-4932: exp(-5000) = 1e-2171 is a normal
number) on head + residual, with the series e - e^2 / 2 for log1p(e) below 1e-19, where 1 + e would have rounded e away.  sigma is
sign-symmetric, e / (1 + e) or 1 / (1 + e), never 1 - sigma.  Relative error: the exponential's argument carries |t| 2^-64 (2.7e-16 at |t| =
5000), everything else a few 2^-64 -- against the float64 bounds below (r = 1e-11) nothing.  pi, L, l are RETURNED as float64 (L and pi
below 2.2e-308 come back subnormal or 0, which the bounds' floor covers); the table's sums run over the longdouble values.

Bounds, per pair (u the unit roundoff, r the relative constant of `dtype`: eval_reference.U, R; s_i = sum_j |x_ij beta_j|):

    delta = (p + 1) u s                          worst-case error of the dot product
    t-    = (|t| - delta)+                       the logit moved toward 0 by delta
    q+    = e / (1 + e)^2 at t-                  |d sigma / dt| is decreasing in |t|: its largest value over the logit's interval
    w+    = sigma(-t- sign t)                    |d l / dt| = sigma(-t), likewise
    floor = the smallest normal number of dtype  (the float32 hardware exponential returns no subnormals, and float64's ldexp loses digits there)
    tol_L  = r L + q+ delta + floor              tol_pi the same with pi: sigma(eta) and sigma(-eta) share q+
    tol_l  = r |l| + w+ delta + 2 u max(t, 0)    (the last term as in eval_reference.bounds: for t > 0, l = -log1p(e) is formed from 1 + e,
                                                  which rounds e at the magnitude of 1)

of the table (v_s the reference's pair values, m their mean, tol_s the pair bounds):

    rows 0, 2, 3     mean_s tol_s
    rows 1, 4        sum_s (2 |v_s - m| tol_s + tol_s^2)  +  (S + 8) 2^-53 (M2 + S max_s (v_s - m)^2)  +  floor64
                     (the second term: the float64 accumulation of the pivot-shifted sums and of the pairwise merge, whose terms are
                      squares of differences no larger than twice the largest deviation.
                      floor64 = 2^-1022, the smallest normal float64 number, whatever the model's dtype -- the sums are float64.  The
                      second term is RELATIVE, and float64 keeps no relative accuracy below 2^-1022: where pi is 1e-157 its squared
                      deviations are subnormal, every d^2 the accumulator forms is rounded to a multiple of 2^-1074 (error up to
                      2^-1075 each, whatever its size), and the merge multiplies such a rounded d^2 by n_a n_b / (n_a + n_b) < S.
                      Fewer than S + 8 such roundings, each weighted by less than S: S (S + 8) 2^-1075, below 2^-1022 for every
                      S < 2^26.  The first GPU run of these tests met it: a row 1 of 3.028252996e-315 against 3.028253e-315, one
                      step of the subnormal grid, under a bound that had underflowed to 0.)

tol_L scales with L, so row 2 is held RELATIVELY wherever every draw's L is small.  No factor multiplies any bound.
"""
import numpy as np

import eval_reference as er

LD = np.longdouble
FLOOR64 = float(np.finfo(np.float64).tiny)
FLOOR = {"float32": float(np.finfo(np.float32).tiny), "float64": float(np.finfo(np.float64).tiny)}
SERIES_BELOW = LD("1e-19")


def _f64(a):
    with np.errstate(under="ignore"):
        return np.asarray(a, dtype=np.float64)


def _sigma_terms(t):
    """t longdouble -> e = exp(-|t|), sigma(t), sigma(-t), log sigma(t), all longdouble."""
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(t))
        rcp = 1 / (1 + e)
        big, small = rcp, e * rcp
        l1p = np.where(e < SERIES_BELOW, e - e * e / 2, np.log1p(e))
    nonneg = t >= 0
    return e, np.where(nonneg, big, small), np.where(nonneg, small, big), np.minimum(t, LD(0)) - l1p


def pairs(X, y, B, dtype):
    """pi, L, l of every pair as a model of `dtype` holds rows X [r, p], labels y [r] (or None) and draws B [S, p].
    -> dict: pi, L, l [S, r] float64 (L and l None without labels); "ld": the same three in longdouble; eta, s [S, r] float64 (eta the
    rounded logit, for the bounds); sign [r] (+1 / -1; +1 without labels); p; dtype."""
    X, B = er.held(X, dtype), np.atleast_2d(er.held(B, dtype))
    th, tl, s = er.logits(X, B)
    eta = th.astype(LD) + tl.astype(LD)
    sign = np.ones(X.shape[0]) if y is None else 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    _, pi, _, _ = _sigma_terms(eta)
    out = dict(pi=_f64(pi), L=None, l=None, ld=dict(pi=pi, L=None, l=None), eta=_f64(eta), s=s, sign=sign, p=X.shape[1], dtype=dtype,
               labels=y is not None)
    if y is not None:
        _, L, _, l = _sigma_terms(eta * sign[None, :].astype(LD))
        out.update(L=_f64(L), l=_f64(l))
        out["ld"].update(L=L, l=l)
    return out


def pair_bounds(ref):
    """dict: pi, L, l [S, r] float64 (L, l None without labels) -- the tolerances of the module docstring."""
    dtype = ref["dtype"]
    u, r, floor = er.U[dtype], er.R[dtype], FLOOR[dtype]
    delta = ((ref["p"] + 1) * u * ref["s"]).astype(LD)
    eta = ref["eta"].astype(LD)
    with np.errstate(under="ignore"):
        e = np.exp(-np.maximum(np.abs(eta) - delta, LD(0)))
        qplus = e / ((1 + e) * (1 + e))
        tol = dict(pi=_f64(r * ref["ld"]["pi"] + qplus * delta + floor), L=None, l=None)
        if ref["labels"]:
            t = eta * ref["sign"][None, :].astype(LD)
            wplus = np.where(t > 0, e / (1 + e), 1 / (1 + e))
            tol["L"] = _f64(r * ref["ld"]["L"] + qplus * delta + floor)
            tol["l"] = _f64(r * np.abs(ref["ld"]["l"]) + wplus * delta + 2 * u * np.maximum(t, LD(0)))
    return tol


def _moments(v):
    m = v.sum(axis=0) / LD(v.shape[0])
    d = v - m[None, :]
    return m, (d * d).sum(axis=0), d


def table(ref):
    """The table [5, r] float64 of the header from the longdouble pair values (two-pass moments); rows 2 - 4 NaN without labels."""
    out = np.full((5, ref["pi"].shape[1]), np.nan)
    m, q, _ = _moments(ref["ld"]["pi"])
    out[0], out[1] = _f64(m), _f64(q)
    if ref["labels"]:
        out[2] = _f64(ref["ld"]["L"].sum(axis=0) / LD(ref["L"].shape[0]))
        m, q, _ = _moments(ref["ld"]["l"])
        out[3], out[4] = _f64(m), _f64(q)
    return out


def table_bounds(ref, tol=None):
    """[5, r] float64 tolerances of the table (NaN in rows 2 - 4 without labels)."""
    tol = pair_bounds(ref) if tol is None else tol
    S = ref["pi"].shape[0]
    out = np.full((5, ref["pi"].shape[1]), np.nan)

    def m2_bound(v, tl):
        _, q, d = _moments(v)
        tl = tl.astype(LD)
        ad = np.abs(d)
        return _f64((2 * ad * tl + tl * tl).sum(axis=0) + (S + 8) * LD(2.0 ** -53) * (q + S * ad.max(axis=0) ** 2)) + FLOOR64
    out[0] = tol["pi"].mean(axis=0)
    out[1] = m2_bound(ref["ld"]["pi"], tol["pi"])
    if ref["labels"]:
        out[2] = _f64(tol["L"].astype(LD).sum(axis=0) / LD(S))
        out[3] = tol["l"].mean(axis=0)
        out[4] = m2_bound(ref["ld"]["l"], tol["l"])
    return out


def ratio(got, ref, tol):
    """Largest |got - ref| / tol over entries that are not NaN on both sides (0 / 0 counts as 0; a NaN or infinity on one side only is
    infinite)."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    both = np.isnan(got) & np.isnan(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        q = np.where(both | (err == 0), 0.0, err / tol)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0
