"""An independent float64 NumPy restatement of the PSIS stage of include/logreg_hip_loo.h -- TEST INFRASTRUCTURE ONLY.

`psis_row(l)` follows the header line by line for one observation's log-likelihoods l_s (sort instead of select, np.sum instead of
fixed trees); `psis_table(loglik)` stacks it over the columns of an `[S, r]` matrix.  `direct_elpd(l, lw)` is the guard of the closed
form: the textbook logsumexp(lw + l) - logsumexp(lw) from the full vector of log weights that `psis_row(..., return_lw=True)` builds.
`loglik_matrix(X, y, B, mode)` is the fill stage: l = min(t, 0) - log1p(exp(-|t|)) per pair in float64 or in float32 arithmetic (the
dot product as a sequential float32 multiply-add chain), as tests/predict_reference.py computes its l.
"""
import math

import numpy as np

LOO_ROWS = 5


def tail_length(S):
    """M = min(floor(S / 5), m3), m3 = the smallest integer with m3^2 >= 9 S"""
    S = int(S)
    if S <= 0:
        return 0
    m3 = math.isqrt(9 * S)
    if m3 * m3 < 9 * S:
        m3 += 1
    return min(S // 5, m3)


def gpd_fit(x):
    """Zhang & Stephens (2009) as in `loo` / arviz, x ascending and positive -> (k after the shrink, sigma)"""
    n = len(x)
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1, dtype=np.float64)
    q = int(math.floor(n / 4 + 0.5))
    theta = 1.0 / x[n - 1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x[q - 1])
    k = np.mean(np.log1p(-theta[:, None] * x[None, :]), axis=1)
    L = n * (np.log(-theta / k) - k - 1.0)
    w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
    theta_hat = np.sum(theta * w)
    k = np.mean(np.log1p(-theta_hat * x))
    sigma = -k / theta_hat
    return (n * k + 5.0) / (n + 10.0), sigma


def psis_row(l, return_lw=False):
    """-> (elpd, khat, n_eff, lppd, n_tail) of one observation; with return_lw also the vector of log weights (unnormalised)"""
    l = np.asarray(l, dtype=np.float64)
    S = l.shape[0]
    if not np.all(np.isfinite(l)):
        out = (np.nan,) * 5
        return (out, np.full(S, np.nan)) if return_lw else out
    with np.errstate(all="ignore"):
        a = np.max(-l)
        v = -l - a
        M = tail_length(S)
        lppd = np.log(np.sum(np.exp(l)) / S)
        raw, khat, n_t = True, np.inf, 0
        w = np.exp(v)
        lw = v.copy()
        num = float(S)
        if M > 0:
            c = np.sort(v)[S - M - 1]
            in_tail = v > c
            n_t = int(np.sum(in_tail))
            if n_t >= 5:
                idx = np.flatnonzero(in_tail)
                idx = idx[np.argsort(v[idx], kind="stable")]
                vt = v[idx]
                ec = np.exp(c)
                k, sigma = gpd_fit(np.exp(vt) - ec)
                if np.isfinite(k) and np.isfinite(sigma):
                    raw, khat = False, k
                    p = (np.arange(1, n_t + 1) - 0.5) / n_t
                    lp = np.log1p(-p)
                    qq = -sigma * lp if k == 0 else sigma / k * (np.exp(-k * lp) - 1.0)
                    wt = np.minimum(ec + qq, 1.0)
                    w[idx] = wt
                    lw[idx] = np.log(wt)
                    num = float(S - n_t) + np.sum(np.exp(np.log(wt) - vt))
        den = np.sum(w[~in_tail]) + np.sum(w[in_tail]) if M > 0 else np.sum(w)
        den2 = np.sum(w[~in_tail] ** 2) + np.sum(w[in_tail] ** 2) if M > 0 else np.sum(w ** 2)
        out = ((np.log(num) - np.log(den)) - a, khat, den * den / den2, lppd, float(n_t))
    return (out, lw) if return_lw else out


def direct_elpd(l, lw):
    """logsumexp(lw + l) - logsumexp(lw)"""
    from scipy.special import logsumexp
    l = np.asarray(l, dtype=np.float64)
    return float(logsumexp(lw + l) - logsumexp(lw))


def psis_table(loglik):
    """[S, r] -> table [5, r] float64"""
    L = np.asarray(loglik, dtype=np.float64)
    return np.array([psis_row(L[:, i]) for i in range(L.shape[1])]).T.copy()


def loglik_matrix(X, y, B, mode="float64"):
    """[S, n]: l of every (draw, row) pair, per-pair arithmetic in `mode`, returned in that dtype"""
    dt = {"float64": np.float64, "float32": np.float32}[mode]
    X = np.ascontiguousarray(X, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt).reshape(-1, X.shape[1])
    sgn = (2 * np.asarray(y, dtype=np.float64) - 1).astype(dt)
    Xs = X * sgn[:, None]
    if dt == np.float64:
        t = B @ Xs.T
    else:
        t = np.zeros((B.shape[0], X.shape[0]), dtype=np.float32)
        for j in range(X.shape[1]):
            t = t + B[:, j:j + 1] * Xs[None, :, j]
    l = np.minimum(t, dt(0)) - np.log1p(np.exp(-np.abs(t)))
    assert l.dtype == dt
    return l
