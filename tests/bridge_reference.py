"""An independent NumPy restatement of bridge sampling as include/logreg_hip_bridge.h defines it -- TEST INFRASTRUCTURE ONLY.

    terms(X, y, pscale, B, mu, cov, mode)     l = lpost - log g per draw, float64; the per-row log-likelihood in `mode` ("float64" |
                                              "float32": np.float32 arithmetic per pair, as tests/loo_reference.py), the row sum, the prior
                                              and the Gaussian in float64 (the Gaussian by forward substitution in np.longdouble)
    proposal_draws(seed, N2, mu, cov, dtype)  mu + L z from Philox4x32-10 + Box-Muller in float64, rounded to dtype
    solve(l1, l2, n_eff, tol, maxit)          the iteration and the error
    quadrature_logml(X, y, pscale, step)      log p(y) of a 2-parameter model on a grid
    term_bound64 / term_unit32                the float64 bound of a term derived from the inputs; the float32 unit

The inputs are taken as given: a caller comparing against a float32 model passes X and B rounded to float32 already.
"""
import numpy as np

import pg_reference as pgr

BRIDGE_TAG = 0x08000000
EPS = float(np.finfo(np.float64).eps)
# The shapes of the terms test (tests/test_gpu_bridge.py): a pad, an exact width and each width boundary; rows below a wave, across a
# 256-row workgroup and across a 512-row slice; draws per call
WIDTHS, ROWS, CALLS = (3, 8, 17, 33, 128), (1, 63, 257, 601), (1, 33, 1025)
# The float32 tolerance of a term, in units of term_unit32 (2^-24 per row of the row's magnitudes), by the number of rows (a term is a sum
# over the rows: the rows' rounding errors cancel as n grows): 8 x the largest deviation of this reference's float32 mode from its float64
# mode over the GPU test's own cases, gpu_term_case(p, n) for p in WIDTHS, and over saturated_case().  tests/test_bridge_cpu.py re-measures
# them.  Largest measured: n = 1: 1.615 (p = 3), 63: 0.156, 257: 0.091, 601: 0.047; saturated: 0.060
F32_UNITS = {1: 13.0, 63: 1.3, 257: 0.75, 601: 0.4, "saturated": 0.5}


# ---- the model's side ---------------------------------------------------------------------------------------------------------------------
def loglik_rows(X, y, B, mode="float64"):
    """[S, n]: l of every (draw, row) pair, per-pair arithmetic in `mode`"""
    dt = {"float64": np.float64, "float32": np.float32}[mode]
    X = np.ascontiguousarray(X, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt).reshape(-1, X.shape[1])
    sgn = (2 * np.asarray(y, dtype=np.float64) - 1).astype(dt)
    Xs = X * sgn[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        if dt == np.float64:
            t = B @ Xs.T
        else:
            t = np.zeros((B.shape[0], X.shape[0]), dtype=np.float32)
            for j in range(X.shape[1]):
                t = t + B[:, j:j + 1] * Xs[None, :, j]
        l = np.minimum(t, dt(0)) - np.log1p(np.exp(-np.abs(t)))
    assert l.dtype == dt
    return l


def lprior(pscale, B):
    ps = np.asarray(pscale, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sum(-np.log(ps) - 0.5 * np.log(2 * np.pi)) - 0.5 * np.sum((B / ps) ** 2, axis=1)


def factor(cov):
    """L (Cholesky, lower) and c_g = -sum log L_ii - p / 2 log(2 pi)"""
    L = np.linalg.cholesky(np.asarray(cov, dtype=np.float64))
    return L, float(-np.sum(np.log(np.diag(L))) - 0.5 * L.shape[0] * np.log(2 * np.pi))


def log_g(B, mu, cov):
    """log N(B_s; mu, cov), [S] float64: L y = d by forward substitution in np.longdouble"""
    L, cg = factor(cov)
    Ll = L.astype(np.longdouble)
    d = (np.asarray(B, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[None, :]).astype(np.longdouble)
    p = L.shape[0]
    yv = np.zeros_like(d)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(p):
            yv[:, i] = (d[:, i] - yv[:, :i] @ Ll[i, :i]) / Ll[i, i]
        return (np.longdouble(cg) - np.longdouble(0.5) * np.sum(yv * yv, axis=1)).astype(np.float64)


def terms(X, y, pscale, B, mu, cov, mode="float64"):
    B = np.asarray(B)
    with np.errstate(over="ignore", invalid="ignore"):
        ll = np.sum(loglik_rows(X, y, B, mode).astype(np.longdouble), axis=1).astype(np.float64)
        return (ll + lprior(pscale, B)) - log_g(B, mu, cov)


def term_bound64(X, pscale, B, mu, cov, few=4.0):
    """The float64 bound of |device term - reference term|, [S], from the inputs: n row terms and p^2 Gaussian terms, each `few` ulp of
    its magnitude.
      row i      the logit: p fused multiply-adds, each within eps / 2 of the running magnitude A_i = sum_j |x_ij theta_j|; l has slope <= 1 in
                 the logit and its own evaluation costs a few ulp of |l| + 1, |l_i| <= A_i + log 2:      p A_i + 4 (|l_i| + 1)
      row sum    a tree of depth <= 16 over the |l_i|:                                                    16 sum_i |l_i|
      prior      p terms of magnitude theta_j^2 / sd_j^2, each counted p times, and the constant
      Gaussian   y_i = sum_j W_ij d_j: (i + 2) ulp of (|W| |d|)_i for the sum, 2 p (|W| |L| |W| |d|)_i for W = L^-1 itself (its backward
                 error), q = sum y_i^2: 2 |y_i| err_i + p q; the two Cholesky factors (LAPACK's and the library's) are exact factors of
                 matrices within p eps |L| |L^T| of cov: 2 p | |L^T| |W^T y| |^2;  c_g: 2 (p + sum |log L_ii|)
    all times eps, and the whole times `few`."""
    Xa, B, ps = np.abs(np.asarray(X, dtype=np.float64)), np.asarray(B, dtype=np.float64), np.asarray(pscale, dtype=np.float64)
    p = Xa.shape[1]
    A = np.abs(B) @ Xa.T  # [S, n]
    prior = p * np.sum((B / ps) ** 2, axis=1) + p + np.sum(np.abs(np.log(ps)))
    return (_bound_parts(B, mu, cov, A, p) + prior) * few * EPS


def _bound_parts(B, mu, cov, A, p):
    L, _ = factor(cov)
    W = np.linalg.inv(L)
    aW, aL = np.abs(W), np.abs(L)
    d = B - np.asarray(mu, dtype=np.float64)[None, :]
    yv = d @ W.T
    Wd = np.abs(d) @ aW.T  # (|W| |d|)_i
    WLWd = Wd @ (aW @ aL).T
    idx = np.arange(p, dtype=np.float64)[None, :] + 2.0
    err_y = idx * Wd + 2.0 * p * WLWd
    q = np.sum(yv * yv, axis=1)
    u = np.abs(yv @ W) @ aL  # |L^T| |W^T y|  (row form)
    gauss = 0.5 * (np.sum(2.0 * np.abs(yv) * err_y, axis=1) + p * q + 2.0 * p * np.sum(u * u, axis=1)) + 2.0 * (p + np.sum(np.abs(np.log(np.diag(L)))))
    # |l_i| <= A_i + log 2
    labs = A + np.log(2.0)
    rows = np.sum(p * A + 4.0 * (labs + 1.0), axis=1) + 16.0 * np.sum(labs, axis=1)
    return rows + gauss


def term_unit32(X, B):
    """[S]: 2^-24 sum_i (sum_j |x_ij theta_j| + 1), one float32 ulp of every row's magnitudes -- the unit of F32_UNITS"""
    A = np.abs(np.asarray(B, dtype=np.float64)) @ np.abs(np.asarray(X, dtype=np.float64)).T
    return 2.0 ** -24 * np.sum(A + 1.0, axis=1)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def term_case(p, n, seed, S=64):
    """A model with unit priors whose posterior-like draws come from a proposal with correlation 0.9 and standard deviations spanning
    10^4: X [n, p] with columns scaled by 1 / sd (logits of order 1), y, pscale, mu, cov, B [S, p] = mu + 1.5 L z."""
    rng = np.random.default_rng(seed)
    sd = np.logspace(-2, 2, p) if p > 1 else np.ones(1)
    X = rng.standard_normal((n, p)) / sd[None, :] / np.sqrt(p)
    y = (rng.random(n) < 0.5).astype(np.float64)
    mu = rng.standard_normal(p) * sd
    R = np.full((p, p), 0.9) + 0.1 * np.eye(p)
    cov = R * np.outer(sd, sd)
    L = np.linalg.cholesky(cov)
    B = mu[None, :] + 1.5 * rng.standard_normal((S, p)) @ L.T
    return {"X": X, "y": y, "pscale": np.ones(p), "mu": mu, "cov": cov, "B": B}


def gpu_term_case(p, n):
    return term_case(p, n, seed=100 * p + n, S=sum(CALLS))


def saturated_case():
    """300 x 5; the first 20 of 40 draws scaled so that the largest logit of each is 5000"""
    rng = np.random.default_rng(3)
    n, p = 300, 5
    X = rng.standard_normal((n, p))
    y = (rng.random(n) < 0.5).astype(np.float64)
    B = rng.standard_normal((40, p))
    B[:20] *= 5000.0 / np.max(np.abs(X @ B[:20].T), axis=0)[:, None]
    return {"X": X, "y": y, "pscale": np.full(p, 1e4), "mu": np.zeros(p), "cov": 4.0 * np.eye(p), "B": B}


def rounded(c, dt):
    """the case as a model of dtype dt sees it: X and B rounded"""
    return dict(c, X=c["X"].astype(dt).astype(np.float64), B=c["B"].astype(dt).astype(np.float64))


def small_model(seed=0):
    """The seeded 30 x 2 model of the quadrature checks"""
    rng = np.random.default_rng(1000 + seed)
    X = np.column_stack([np.ones(30), rng.standard_normal(30)])
    eta = X @ np.array([0.5, -1.0])
    y = (rng.random(30) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return X, y, np.array([2.0, 2.0])


def lpost64(X, y, pscale, B):
    B = np.asarray(B, dtype=np.float64).reshape(-1, X.shape[1])
    return np.sum(loglik_rows(X, y, B), axis=1) + lprior(pscale, B)


def newton_mode(X, y, pscale, iters=50):
    """(mode, covariance of the Laplace approximation) by Newton's method in float64"""
    X, y, ps = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(pscale, dtype=np.float64)
    b = np.zeros(X.shape[1])
    for _ in range(iters):
        pi = 1.0 / (1.0 + np.exp(-(X @ b)))
        g = X.T @ (y - pi) - b / ps ** 2
        H = (X * (pi * (1 - pi))[:, None]).T @ X + np.diag(1.0 / ps ** 2)
        step = np.linalg.solve(H, g)
        b = b + step
        if np.max(np.abs(step)) < 1e-13:
            break
    return b, np.linalg.inv(H)


def quadrature_logml(X, y, pscale, step=0.01, half=8.0):
    """log INT exp(lpost) over a grid of `step` around the mode, +-`half` Laplace standard deviations (2 parameters)"""
    b, C = newton_mode(X, y, pscale)
    sd = np.sqrt(np.diag(C))
    g0 = np.arange(b[0] - half * sd[0], b[0] + half * sd[0] + step, step)
    g1 = np.arange(b[1] - half * sd[1], b[1] + half * sd[1] + step, step)
    tot = -np.inf
    for a in g0:  # a grid line at a time
        lp = lpost64(X, y, pscale, np.column_stack([np.full(g1.size, a), g1]))
        m = np.max(lp)
        tot = np.logaddexp(tot, m + np.log(np.sum(np.exp(lp - m))))
    return float(tot + 2.0 * np.log(step))


def importance_logml(X, y, pscale, N, seed=0, scale=1.5):
    """(log p(y), its standard error, the effective size) from N draws of N(mode, scale^2 x the Laplace covariance), float64"""
    b, C = newton_mode(X, y, pscale)
    cov = scale ** 2 * C
    L = np.linalg.cholesky(cov)
    rng = np.random.default_rng(seed)
    lw = np.empty(N)
    for i0 in range(0, N, 50000):
        th = b[None, :] + rng.standard_normal((min(50000, N - i0), b.size)) @ L.T
        lw[i0:i0 + th.shape[0]] = lpost64(X, y, pscale, th) - log_g(th, b, cov)
    m = np.max(lw)
    w = np.exp(lw - m)
    return float(m + np.log(np.mean(w))), float(np.std(w, ddof=1) / (np.mean(w) * np.sqrt(N))), float(np.sum(w) ** 2 / np.sum(w * w))


# ---- the proposal draws ------------------------------------------------------------------------------------------------------------------
def proposal_normals(seed, j, p):
    """z [len(j), p]: Philox4x32-10, key = seed, counter = (j lo, j hi, 0, BRIDGE_TAG | b), Box-Muller pairs (w0, w1), (w2, w3), float64"""
    j = np.atleast_1d(np.asarray(j, dtype=np.uint64))
    nb = (p + 3) // 4
    blk = (np.arange(nb, dtype=np.uint64) | np.uint64(BRIDGE_TAG))[None, :]
    w = pgr.philox((j & np.uint64(0xFFFFFFFF))[:, None], (j >> np.uint64(32))[:, None], 0, blk, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    z = np.empty((j.size, nb, 4))
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(pgr._u(w[2 * h], np.float64)))
        th = 2.0 * np.pi * pgr._u(w[2 * h + 1], np.float64)
        z[:, :, 2 * h], z[:, :, 2 * h + 1] = r * np.cos(th), r * np.sin(th)
    return z.reshape(j.size, nb * 4)[:, :p]


def proposal_draws(seed, N2, mu, cov, dtype=np.float64):
    L, _ = factor(cov)
    z = proposal_normals(seed, np.arange(N2), L.shape[0])
    return (np.asarray(mu, dtype=np.float64)[None, :] + z @ L.T).astype(dtype)


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
def solve(l1, l2, n_eff=None, tol=1e-10, maxit=1000):
    """-> dict(logml, se, iterations, converged, n_eff, n_nonfinite, trace): the header's iteration in float64 NumPy.  trace: log r
    after the start and after every iteration."""
    l1, l2 = np.asarray(l1, dtype=np.float64), np.asarray(l2, dtype=np.float64)
    N1, N2 = l1.size, l2.size
    neff = float(N1) if n_eff is None or not n_eff > 0 else float(n_eff)
    bad = int(np.sum(~np.isfinite(l1)) + np.sum(~np.isfinite(l2)))
    out = {"n_eff": neff, "n_nonfinite": bad, "iterations": 0, "converged": False, "logml": np.nan, "se": np.nan, "trace": []}
    if bad:
        return out
    s1, s2 = neff / (neff + N2), N2 / (neff + N2)
    ls1, ls2 = np.log(s1), np.log(s2)
    max2, min1 = np.max(l2), np.min(l1)
    lr = max2 + (np.log(np.sum(np.exp(l2 - max2))) - np.log(N2))
    trace = [lr]
    it, conv = 0, False
    while it < maxit and not conv:
        c = ls2 + lr
        top2 = max2 - np.logaddexp(ls1 + max2, c)
        top1 = -np.logaddexp(ls1 + min1, c)
        sum2 = np.sum(np.exp((l2 - np.logaddexp(ls1 + l2, c)) - top2))
        sum1 = np.sum(np.exp(-np.logaddexp(ls1 + l1, c) - top1))
        new = max2 + (np.logaddexp(ls1 + min1, c) - np.logaddexp(ls1 + max2, c)) + ((np.log(sum2) - np.log(N2)) - (np.log(sum1) - np.log(N1)))
        it += 1
        conv = abs(new - lr) <= tol * max(1.0, abs(new))
        lr = new
        trace.append(lr)
    with np.errstate(over="ignore"):
        f1 = 1.0 / (s1 + s2 * np.exp(lr - l2))  # p / (s1 p + s2 g) over the proposal terms
        f2 = 1.0 / (s1 * np.exp(l1 - lr) + s2)  # g / (s1 p + s2 g) over the posterior terms
    v1 = np.var(f1, ddof=1) if N2 > 1 else 0.0
    v2 = np.var(f2, ddof=1) if N1 > 1 else 0.0
    re2 = v1 / (np.mean(f1) ** 2 * N2) + v2 / (np.mean(f2) ** 2 * neff)
    out.update(logml=float(lr), se=float(np.sqrt(re2)), iterations=it, converged=bool(conv), trace=trace)
    return out


# ---- the Pima fixture (tests/golden/bridge_pima.json): `python tests/bridge_reference.py` rewrites it -----------------------------------------
PIMA_DROP = 3  # the column left out of the smaller design


def make_pima_fixture(N=600000):
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "pima_xy.json")) as f:
        d = json.load(f)
    X, y = np.array(d["X"]), np.array(d["y"])
    pscale = np.array([10.0, 1, 1, 1, 1, 1, 1, 1])
    keep = [j for j in range(X.shape[1]) if j != PIMA_DROP]
    full = importance_logml(X, y, pscale, N, seed=1)
    sub = importance_logml(X[:, keep], y, pscale[keep], N, seed=2)
    out = {"what": "log p(y) of the Pima model by a float64 NumPy importance sampler around the Newton mode (proposal: 1.5^2 x the Laplace "
                   "covariance); `dropped`: the design without column `drop`", "draws": N, "drop": PIMA_DROP,
           "full": {"logml": full[0], "se": full[1], "ess": full[2]}, "dropped": {"logml": sub[0], "se": sub[1], "ess": sub[2]},
           "log_bf_full_vs_dropped": full[0] - sub[0]}
    with open(os.path.join(golden, "bridge_pima.json"), "w") as f:
        json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    print(make_pima_fixture())
