"""Independent NumPy statement of include/logreg_hip_cov.h -- TEST INFRASTRUCTURE ONLY.  Nothing is shared with the library or with
logreg_amd/covariance.py.

Tables.  u = (x - center) * scale in float64 exactly as the header spells it, then every sum in EXTENDED PRECISION, np.longdouble with a
64-bit significand (asserted): moment = U^T U over the N = n C draws, chain_sums = the sum over time per chain, sum and chain_outer from
the extended-precision chain sums.  A product of two doubles rounded to 64 bits and N additions in 64 bits err by at most
(N + 1) 2^-64 T: 2^-11 = 0.05 % of the bounds below, which are 2^-53 times the same T.

Forward-error bounds, from the inputs alone (they ARE the tolerances of tests/test_gpu_cov.py).  eps = 2^-53:

    moment[i][j]      (N + 4) eps T + 4 eps T,  T = sum |u_i u_j| over the N draws: N fma in any order, and the two roundings of each u
    chain_sums[c][j]  (n + 2) eps sum_t |u|                    sum[j]   (N + 2) eps sum |u| over the N draws
    chain_outer[i][j] sum_c (|S_ci| dS_cj + |S_cj| dS_ci) + (C + 4) eps sum_c |S_ci S_cj|,  dS = the chain-sum bound

An entry is finite exactly where every draw that enters it is: a NaN or an inf in coordinate j makes S[c][j] of its chain, sum[j] and
rows and columns j of moment and chain_outer non-finite, and nothing else.

Derived figures (`derived`, `derived_bounds`): the covariance, correlation, W, B and lambda_max computed directly from the draws of the
finite coordinates (np.cov, np.corrcoef in float64 on draws centred and scaled by their own mean and sd first, so that their own
rounding is of the size the bounds describe), and the first-order propagation of the table bounds through
logreg_amd.covariance.result_from_tables.  With A = M - s s^T / N, d = 1 / scale:

    dA_ij   = dM_ij + (|s_i| ds_j + |s_j| ds_i) / N + 4 eps (|M_ij| + |s_i s_j| / N)
    cov     = A d_i d_j / (N - 1)                   tol = 1.01 (dA + 6 eps |A|) d_i d_j / (N - 1)
    cor     = A_ij / sqrt(A_ii A_jj)                tol = 1.01 (dA_ij / sqrt(A_ii A_jj) + |cor| (dA_ii / A_ii + dA_jj / A_jj) / 2 + 4 eps |cor|)
    mean    = center + d s / N                      tol = d ds / N + 4 eps (|center| + d |s| / N)
    W (u)   = (M - Q / n) / (C (n - 1))             dW  = (dM + dQ / n + 4 eps (|M| + |Q| / n)) / (C (n - 1))
    B (u)   = (Q / n - s s^T / N) / (C - 1)         dB  = (dQ / n + (|s_i| ds_j + |s_j| ds_i) / N + 6 eps (|Q| / n + |s_i s_j| / N)) / (C - 1)
    lambda  = lambda_max(W^-1 B / n)                tol = 1.01 (|dB / n|_F + lambda |dW|_F) / lambda_min(W)      (Weyl, first order)
                                                          + 16 p eps (|B / n|_F + lambda |W|_F) / lambda_min(W)  (the two eigen-solvers)
(1.01: the second-order terms.)  The direct figures carry a bound of the same form for their own float64 sums, so a comparison uses
twice the tolerance.
"""
import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"


def tables(x, center, scale):
    """x [n, C, p] float64 (already rounded to the dtype under test) -> dict: moment, chain_outer [p, p], sum [p], chain_sums [C, p] and
    tol_<name> of the same shapes (float64; non-finite where the table is), finite [p] bool."""
    x = np.asarray(x, dtype=np.float64)
    center, scale = np.asarray(center, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    n, C, p = x.shape
    N = n * C
    e = LD(EPS)
    with np.errstate(invalid="ignore", over="ignore"):
        u64 = (x - center) * scale  # float64 operations, as the header spells them
        finite = np.all(np.isfinite(u64), axis=(0, 1))
        U = u64.astype(LD)
        A = np.abs(U)
        F, FA = U.reshape(N, p), A.reshape(N, p)
        M = F.T @ F
        T = FA.T @ FA
        S = U.sum(axis=0)              # [C, p]
        SA = A.sum(axis=0)
        s, sa = S.sum(axis=0), SA.sum(axis=0)
        Q = S.T @ S
        dS = (n + 2) * e * SA
        absS = np.abs(S)
        dQ = absS.T @ dS + dS.T @ absS + (C + 4) * e * (absS.T @ absS)
        out = {"moment": M, "tol_moment": (N + 8) * e * T, "chain_sums": S, "tol_chain_sums": dS, "sum": s, "tol_sum": (N + 2) * e * sa,
               "chain_outer": Q, "tol_chain_outer": dQ}
    # non-finite exactly where a non-finite draw enters (long double arithmetic gives this by itself; stated here as the rule)
    series = np.all(np.isfinite(u64), axis=0)  # [C, p]
    pair = finite[:, None] & finite[None, :]
    want = {"moment": pair, "chain_outer": pair, "sum": finite, "chain_sums": series}
    res = {"n": n, "C": C, "p": p, "finite": finite}
    for name in ("moment", "chain_outer", "sum", "chain_sums"):
        v, t = np.asarray(out[name], dtype=np.float64), np.asarray(out["tol_" + name], dtype=np.float64)
        assert np.array_equal(np.isfinite(v), want[name]), name
        res[name], res["tol_" + name] = v, np.where(want[name], t, np.nan)
    return res


def compare(got, ref):
    """got = (moment, chain_outer, sum, chain_sums) -> (largest error / bound, list of complaints).  An entry is finite exactly where
    the reference's is; moment and chain_outer are symmetric to the bit."""
    bad, worst = [], 0.0
    for name, g in zip(("moment", "chain_outer", "sum", "chain_sums"), got):
        g = np.asarray(g)
        want, tol = ref[name], ref["tol_" + name]
        if g.shape != want.shape or g.dtype != np.float64:
            bad.append(f"{name}: shape {g.shape} {g.dtype}")
            continue
        if g.ndim == 2 and name != "chain_sums" and g.tobytes() != np.ascontiguousarray(g.T).tobytes():
            bad.append(f"{name}: not symmetric")
        if not np.array_equal(np.isfinite(g), np.isfinite(want)):
            bad.append(f"{name}: finite in {int(np.isfinite(g).sum())} entries, the reference in {int(np.isfinite(want).sum())}, "
                       f"{int(np.sum(np.isfinite(g) != np.isfinite(want)))} differ")
            continue
        ok = np.isfinite(want)
        if not ok.any():
            continue
        err, t = np.abs(g[ok] - want[ok]), tol[ok]
        exact = t == 0
        if np.any(err[exact] != 0):
            bad.append(f"{name}: entries with bound 0 differ (largest {err[exact].max():.3e})")
        if np.any(~exact):
            ratio = float(np.max(err[~exact] / t[~exact]))
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append(f"{name}: error / bound = {ratio:.3e}")
    return worst, bad


def derived(x):
    """Directly from the draws x [n, C, q] (finite): dict of mean, cov, cor (np.cov / np.corrcoef of the pooled draws), within, between,
    rhat, lam = lambda_max(W^-1 B / n) (NaN unless C >= 2, n >= 2 and W is positive definite), rhat_mv."""
    x = np.asarray(x, dtype=np.float64)
    n, C, q = x.shape
    N = n * C
    X = x.reshape(N, q)
    mean = np.asarray(X.astype(LD).mean(axis=0), dtype=np.float64)
    sd = X.std(axis=0)
    sd = np.where(sd > 0, sd, 1.0)
    Z = (x - mean) / sd  # centred and scaled by the draws' own figures: the float64 sums below then round like the library's
    with np.errstate(invalid="ignore", divide="ignore"):
        covz = np.atleast_2d(np.cov(Z.reshape(N, q), rowvar=False)) if N > 1 else np.full((q, q), np.nan)
        cor = np.atleast_2d(np.corrcoef(Z.reshape(N, q), rowvar=False)) if N > 1 else np.full((q, q), np.nan)
        DD = np.outer(sd, sd)
        cm = Z.mean(axis=0)  # [C, q] chain means
        W = sum(np.atleast_2d(np.cov(Z[:, c], rowvar=False)) for c in range(C)) / C if n > 1 else np.full((q, q), np.nan)
        B = n * np.atleast_2d(np.cov(cm, rowvar=False)) if C > 1 else np.full((q, q), np.nan)
        lam = np.nan
        if C >= 2 and n >= 2 and C * (n - 1) >= q and np.all(np.isfinite(W)) and np.linalg.eigvalsh(W)[0] > 0:
            lam = float(np.max(np.linalg.eigvals(np.linalg.solve(W, B / n)).real))
        w, b = np.diag(W), np.diag(B)
        rhat = np.sqrt(((n - 1) / n * w + b / n) / w)
    return {"mean": mean, "cov": covz * DD, "cor": cor, "within": W * DD, "between": B * DD, "rhat": rhat, "lam": lam,
            "rhat_mv": (n - 1) / n + (C + 1) / C * lam, "Wz": W, "Bz": B}


def derived_bounds(ref, J, center, scale):
    """The first-order propagation of the table bounds of `ref` (from `tables`) through result_from_tables, on the coordinates J (all
    finite) -> dict tol_mean, tol_cov, tol_cor, tol_within, tol_between, tol_lam (float64)."""
    J = np.asarray(J)
    n, C = ref["n"], ref["C"]
    N = n * C
    ix = np.ix_(J, J)
    M, dM, Q, dQ = ref["moment"][ix], ref["tol_moment"][ix], ref["chain_outer"][ix], ref["tol_chain_outer"][ix]
    s, ds = ref["sum"][J], ref["tol_sum"][J]
    d = 1.0 / np.asarray(scale, dtype=np.float64)[J]
    c = np.asarray(center, dtype=np.float64)[J]
    DD = np.outer(d, d)
    ss = np.abs(np.outer(s, s))
    cross = np.outer(np.abs(s), ds) + np.outer(ds, np.abs(s))
    with np.errstate(invalid="ignore", divide="ignore"):
        A = M - np.outer(s, s) / N
        dA = dM + cross / N + 4 * EPS * (np.abs(M) + ss / N)
        a, da = np.diag(A), np.diag(dA)
        root = np.sqrt(np.outer(a, a))
        cor = A / root
        out = {"tol_mean": d * ds / N + 4 * EPS * (np.abs(c) + d * np.abs(s) / N),
               "tol_cov": 1.01 * (dA + 6 * EPS * np.abs(A)) * DD / (N - 1),
               "tol_cor": 1.01 * (dA / root + np.abs(cor) * (np.add.outer(da / a, da / a)) / 2 + 4 * EPS * np.abs(cor))}
        Wu = (M - Q / n) / (C * (n - 1.0)) if n > 1 else np.full_like(M, np.nan)
        dW = (dM + dQ / n + 4 * EPS * (np.abs(M) + np.abs(Q) / n)) / (C * (n - 1.0)) if n > 1 else np.full_like(M, np.nan)
        Bu = (Q / n - np.outer(s, s) / N) / (C - 1.0) if C > 1 else np.full_like(M, np.nan)
        dB = (dQ / n + cross / N + 6 * EPS * (np.abs(Q) / n + ss / N)) / (C - 1.0) if C > 1 else np.full_like(M, np.nan)
        out["tol_within"], out["tol_between"] = 1.01 * (dW + 4 * EPS * np.abs(Wu)) * DD, 1.01 * (dB + 4 * EPS * np.abs(Bu)) * DD
        tol_lam = np.nan
        if n > 1 and C > 1 and np.all(np.isfinite(Wu)) and np.all(np.isfinite(Bu)):
            lmin = np.linalg.eigvalsh(Wu)[0]
            if lmin > 0:
                lam = float(np.max(np.linalg.eigvals(np.linalg.solve(Wu, Bu / n)).real))
                fro = np.linalg.norm
                tol_lam = (1.01 * (fro(dB / n) + lam * fro(dW)) + 16 * len(J) * EPS * (fro(Bu / n) + lam * fro(Wu))) / lmin
        out["tol_lam"] = float(tol_lam)
    return out
