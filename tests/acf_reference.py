"""Independent NumPy statement of include/logreg_hip_acf.h -- TEST INFRASTRUCTURE ONLY.

Direct, globally centred sums in np.longdouble: no FFT, no pivot, no streaming, nothing shared with the library or with
logreg_amd/diagnostics.py.  Per series (chain c, coordinate j) of n values, with m the mean:

    acov[l] = (1/n) sum_{t < n-l} (x_t - m)(x_{t+l} - m)   (0 for l >= n)        rho = acov / acov[0]
    Gamma_j = rho[2j] + rho[2j+1], j < min((K+1)/2, n // 2), truncated at the first Gamma_j <= 0
    tau = -1 + 2 sum of the kept Gamma_j;  ESS = n / tau;  ESS = n when n < 4, acov[0] <= 0 or tau <= 0
    capped: no Gamma_j <= 0 within the available pairs AND (K+1)/2 < n // 2 (the stop was K, not the length of the series)
    a series with a NaN or an inf: acov = NaN, ESS = NaN, counted in row 2

Forward-error bounds, computed from the inputs alone (they ARE the tolerances of tests/test_gpu_acf.py).  With u = 2^-53, the pivoted
values xs_t = x_t - x_0, ms their mean, A_l = sum |xs_t xs_{t+l}|, B = sum |xs_t|:

    tol_acov[l] = 4 (n + 16) u (A_l + 4 |ms| B + n ms^2) / n

the standard gamma_n bound of the three sums the streaming form combines (lag sum, the head / tail sums times the mean, the squared
mean); the factor 4 allows any legal ordering of the final combination.  Propagated over the lags of the pairs used:

    d rho_l = (tol_acov[l] + |rho_l| tol_acov[0]) / acov[0]          d Gamma_j = d rho_2j + d rho_2j+1
    d tau   = 2 sum of d Gamma_j over the kept pairs                  d ESS = n d tau / tau^2

A sum over C chains of values v_c with bounds b_c is allowed  sum b_c + C u sum |v_c|  (any summation order: gamma_{C-1}).

The truncation index is discontinuous in Gamma (and ESS in tau at 0): `margin` is the smallest |Gamma_j| / d Gamma_j over every pair up
to and including the truncation pair, and |tau| / d tau -- the test set must keep it above 1e3 for every finite series that is scanned
(a series with n < 4 or acov[0] <= 0 has ESS = n by rule and no Gamma: its margin is inf).
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def reference(x, K):
    """x [n, C, p] float64 (already rounded to the dtype under test), K odd -> dict of float64 arrays:
    acov, tol_acov [K+1, C, p]; ess, tol_ess, margin [C, p]; capped, nan [C, p] bool; trunc [C, p] (kept pairs; -1: no scan);
    sums, tol_sums [K+4, p] (rows as the library's table)."""
    x = np.asarray(x, dtype=np.float64)
    n, C, p = x.shape
    assert K % 2 == 1 and K >= 1
    NS = C * p
    X = x.reshape(n, NS)
    finite = np.all(np.isfinite(X), axis=0)
    L = np.where(finite[None, :], X, 0.0).astype(LD)
    d = L - L.sum(axis=0) / n
    Lt = L - L[0]
    mt = Lt.sum(axis=0) / n
    B = np.abs(Lt).sum(axis=0)
    acov = np.zeros((K + 1, NS), dtype=LD)
    A = np.zeros((K + 1, NS), dtype=LD)
    for l in range(min(K, n - 1) + 1):
        acov[l] = (d[:n - l] * d[l:]).sum(axis=0) / n
        A[l] = np.abs(Lt[:n - l] * Lt[l:]).sum(axis=0)
    tol = 4 * (n + 16) * LD(U) * (A + 4 * np.abs(mt) * B + n * mt * mt) / n
    ess = np.full(NS, float(n), dtype=LD)
    tol_ess = np.zeros(NS, dtype=LD)
    margin = np.full(NS, np.inf)
    capped = np.zeros(NS, dtype=bool)
    trunc = np.full(NS, -1, dtype=np.int64)
    pairs = min((K + 1) // 2, n // 2)
    for s in range(NS):
        if not finite[s]:
            ess[s] = tol_ess[s] = margin[s] = np.nan
            acov[:, s] = tol[:, s] = np.nan
            continue
        if n < 4 or not acov[0, s] > 0:
            continue
        rho = acov[:, s] / acov[0, s]
        drho = (tol[:, s] + np.abs(rho) * tol[0, s]) / acov[0, s]
        gam = rho[0:2 * pairs:2] + rho[1:2 * pairs:2]
        dgam = drho[0:2 * pairs:2] + drho[1:2 * pairs:2]
        nonpos = np.nonzero(gam <= 0)[0]
        k = int(nonpos[0]) if nonpos.size else pairs
        capped[s] = nonpos.size == 0 and (K + 1) // 2 < n // 2
        trunc[s] = k
        tau = -1 + 2 * gam[:k].sum()
        dtau = 2 * dgam[:k].sum()
        upto = min(k + 1, pairs)
        margin[s] = float(min(np.min(np.abs(gam[:upto]) / dgam[:upto]), abs(tau) / dtau if dtau > 0 else np.inf))
        if tau > 0:
            ess[s] = n / tau
            tol_ess[s] = n * dtau / (tau * tau)
    rows = K + 4
    V = np.zeros((rows, NS), dtype=LD)
    Vt = np.zeros((rows, NS), dtype=LD)
    V[0], V[1], V[2], V[3:] = ess, capped, ~finite, acov
    Vt[0], Vt[3:] = tol_ess, tol
    V3, Vt3 = V.reshape(rows, C, p), Vt.reshape(rows, C, p)
    sums = V3.sum(axis=1)
    tol_sums = Vt3.sum(axis=1) + C * LD(U) * np.abs(V3).sum(axis=1)
    f64 = lambda a, shape: np.asarray(a, dtype=np.float64).reshape(shape)  # noqa: E731
    return {"n": n, "K": K, "acov": f64(acov, (K + 1, C, p)), "tol_acov": f64(tol, (K + 1, C, p)), "ess": f64(ess, (C, p)),
            "tol_ess": f64(tol_ess, (C, p)), "margin": margin.reshape(C, p), "capped": capped.reshape(C, p), "nan": (~finite).reshape(C, p),
            "trunc": trunc.reshape(C, p), "sums": f64(sums, (rows, p)), "tol_sums": f64(tol_sums, (rows, p))}


def compare(sums, ess_chain, ref):
    """-> (largest error / bound over the finite entries of the table and of the per-chain ESS, list of complaints).  Counts (rows 1, 2)
    must agree exactly, NaN must sit exactly where the reference has it, an entry whose bound is 0 must agree exactly."""
    bad = []
    sums, ess_chain = np.asarray(sums), np.asarray(ess_chain)
    if sums.shape != ref["sums"].shape or ess_chain.shape != ref["ess"].shape:
        return np.inf, [f"shapes {sums.shape} {ess_chain.shape}"]
    if not np.array_equal(sums[1:3], ref["sums"][1:3]):
        bad.append(f"counts {sums[1:3].tolist()} != {ref['sums'][1:3].tolist()}")
    worst = 0.0
    for name, got, want, tol in (("sums", sums, ref["sums"], ref["tol_sums"]), ("ess_chain", ess_chain, ref["ess"], ref["tol_ess"])):
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            bad.append(f"{name}: NaN pattern differs")
            continue
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok])
        t = tol[ok]
        exact = t == 0
        if np.any(err[exact] != 0):
            bad.append(f"{name}: {int(np.sum(err[exact] != 0))} entries with bound 0 differ (largest {err[exact].max():.3e})")
        if np.any(~exact):
            ratio = float(np.max(err[~exact] / t[~exact]))
            worst = max(worst, ratio)
            if ratio > 1.0:
                bad.append(f"{name}: error / bound = {ratio:.3e}")
    return worst, bad
