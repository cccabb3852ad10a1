"""An independent NumPy restatement of the posterior-predictive table of include/logreg_hip_predict.h -- TEST INFRASTRUCTURE ONLY.

For rows X [r, p], labels y [r] in {0, 1} (or None) and draws B [S, p]:

    eta = x_i . beta_s     pi = sigma(eta)     t = (2 y_i - 1) eta     L = sigma(t)     l = log sigma(t) = min(t, 0) - log1p(exp(-|t|))

    row 0  mean_s pi        row 1  sum_s (pi - mean)^2        row 2  mean_s L        row 3  mean_s l        row 4  sum_s (l - mean)^2

Two modes:
    "float64"  every per-pair value in float64; means and sums of squares TWO-PASS in np.longdouble (80-bit on x86: the sums carry
               11 more bits than the values, so the table is the correctly rounded one for all practical purposes)
    "float32"  every per-pair value in np.float32 arithmetic (the dot product as a sequential float32 multiply-add chain, exp / log1p /
               division in float32), the same longdouble accumulation -- what ANY float32 evaluation of the formulae costs against
               float64: the yardstick of a float32 model's table

The inputs are taken as given: a caller comparing against a float32 model passes X and B rounded to float32 already.
`brute_force_table` is the guard of this file itself: the same table from scipy.special (expit, logsumexp) and np.mean / np.var over the
full [S, r] matrices, with another formula for l (-logaddexp(0, -t)).
"""
import numpy as np

PRED_ROWS = 5


def _pairs(Xb, yb, B, dt):
    """pi, L, l as [S, rb] arrays of dtype dt for the row block Xb [rb, p]"""
    S, p = B.shape
    if dt == np.float64:
        eta = B @ Xb.T
    else:  # a float32 chain, one coordinate at a time
        eta = np.zeros((S, Xb.shape[0]), dtype=np.float32)
        for j in range(p):
            eta = eta + B[:, j:j + 1] * Xb[None, :, j]
        assert eta.dtype == np.float32
    sgn = (2 * yb - 1).astype(dt) if yb is not None else np.ones(Xb.shape[0], dtype=dt)
    t = eta * sgn[None, :]
    one = dt(1)

    def sigma(v):
        e = np.exp(-np.abs(v))
        return np.where(v >= 0, one / (one + e), e / (one + e))
    pi, L = sigma(eta), sigma(t)
    l = np.minimum(t, dt(0)) - np.log1p(np.exp(-np.abs(t)))
    assert pi.dtype == dt and L.dtype == dt and l.dtype == dt
    return pi, L, l


def reference_table(X, y, B, mode="float64", block_pairs=1 << 22, return_info=False):
    """-> table [5, r] float64 (rows 2 - 4 NaN when y is None); with return_info also {"min_L": the smallest per-pair likelihood} --
    a caller asserts on it that row 2 is free of underflow."""
    dt = {"float64": np.float64, "float32": np.float32}[mode]
    X = np.ascontiguousarray(X, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt)
    if B.ndim == 3:
        B = B.reshape(-1, B.shape[-1])
    r, p = X.shape
    S = B.shape[0]
    assert B.shape[1] == p and S >= 1 and r >= 1
    yv = None if y is None else np.asarray(y, dtype=np.float64)
    out = np.full((PRED_ROWS, r), np.nan)
    min_L = np.inf
    rb = max(1, block_pairs // S)
    ld = np.longdouble
    for i0 in range(0, r, rb):
        i1 = min(r, i0 + rb)
        pi, L, l = _pairs(X[i0:i1], None if yv is None else yv[i0:i1], B, dt)

        def moments(v):
            v = v.astype(ld)
            mean = v.sum(axis=0) / ld(S)
            d = v - mean[None, :]
            return mean.astype(np.float64), (d * d).sum(axis=0).astype(np.float64)
        out[0, i0:i1], out[1, i0:i1] = moments(pi)
        if yv is not None:
            out[2, i0:i1] = (L.astype(ld).sum(axis=0) / ld(S)).astype(np.float64)
            out[3, i0:i1], out[4, i0:i1] = moments(l)
            min_L = min(min_L, float(L.min()))
    if return_info:
        return out, {"min_L": min_L}
    return out


def brute_force_table(X, y, B):
    """The table from library functions over the full [S, r] matrices (small cases only)."""
    from scipy.special import expit, logsumexp
    X = np.asarray(X, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64).reshape(-1, X.shape[1])
    S = B.shape[0]
    eta = np.einsum("sj,ij->si", B, X)
    t = eta * (2 * np.asarray(y, dtype=np.float64) - 1)[None, :]
    pi = expit(eta)
    logL = -np.logaddexp(0.0, -t)
    return np.stack([pi.mean(axis=0), pi.var(axis=0) * S, np.exp(logsumexp(logL, axis=0) - np.log(S)), logL.mean(axis=0),
                     logL.var(axis=0) * S])


def posterior_like_draws(X, y, pscale, S, seed, center=None):
    """S draws from the Laplace approximation N(beta_hat, H^-1) of the posterior of (X, y, N(0, pscale^2) priors): posterior-like input
    for the tests without running a sampler.  beta_hat by Newton's method from `center` (default 0)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    p = X.shape[1]
    iv = 1.0 / np.broadcast_to(np.asarray(pscale, dtype=np.float64), (p,)) ** 2
    b = np.zeros(p) if center is None else np.array(center, dtype=np.float64)
    for _ in range(50):
        mu = 1.0 / (1.0 + np.exp(-(X @ b)))
        g = X.T @ (y - mu) - iv * b
        H = (X * (mu * (1 - mu))[:, None]).T @ X + np.diag(iv)
        step = np.linalg.solve(H, g)
        b = b + step
        if np.max(np.abs(step)) < 1e-12:
            break
    Lc = np.linalg.cholesky(np.linalg.inv(H))
    rng = np.random.default_rng(seed)
    return b[None, :] + rng.standard_normal((S, p)) @ Lc.T
