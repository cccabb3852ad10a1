"""Independent NumPy statement of include/logreg_hip_marginals.h -- TEST INFRASTRUCTURE ONLY.  Nothing is shared with the library or with
logreg_amd/marginals.py.

Counts: the header's bin rule, in float64: t = (x - lo) * (B / (hi - lo)); NaN -> column B + 2, t < 0 -> 0, t >= B or x >= hi -> B + 1, else
1 + floor(t).  min / max: np.nanmin / np.nanmax.  Power sums: u = (x - c) * s in float64 exactly as the header spells it
(c = (lo + hi) / 2, s = 2 / (hi - lo)), then S_k = sum u^k in np.longdouble.  Moments (mean, variance with ddof = 1, skewness, kurtosis as
scipy.stats.describe): two passes in np.longdouble over the dtype-rounded draws themselves -- no u, no grid.

Forward-error bounds, from the inputs alone (they ARE the tolerances of tests/test_gpu_marginals.py).  With eps = 2^-53, N = n C draws
of a coordinate and A_k = sum |u|^k:

    tol_S[k] = (N + 4) eps A_k              any order of the N additions, the rounded product u*u of S3 (one) and S4 (two roundings)

Skewness and kurtosis do not change under x -> (x - c) s, whatever c and s are, so the library's figures differ from the two-pass ones by
the roundings only.  E_k = tol_S[k] + 2 k eps A_k (the two roundings of u itself); raw moments a_k = S_k / N with da_k = E_k / N +
eps |a_k|; then, to first order,

    m2 = a2 - a1^2                          dm2 = da2 + 2 |a1| da1 + 3 eps (|a2| + a1^2)
    m3 = a3 - 3 a1 a2 + 2 a1^3              dm3 = da3 + 3 (|a2| da1 + |a1| da2) + 6 a1^2 da1 + 4 eps (|a3| + 3 |a1 a2| + 2 |a1|^3)
    m4 = a4 - 4 a1 a3 + 6 a1^2 a2 - 3 a1^4  dm4 = da4 + 4 (|a3| da1 + |a1| da3) + 6 (2 |a1 a2| da1 + a1^2 da2) + 12 |a1|^3 da1
                                                  + 5 eps (|a4| + 4 |a1 a3| + 6 a1^2 |a2| + 3 a1^4)
    tol_skew = 1.01 (dm3 / m2^1.5 + 1.5 |m3| dm2 / m2^2.5 + 4 eps |skew|)
    tol_kurt = 1.01 (dm4 / m2^2 + 2 |m4| dm2 / m2^3 + 4 eps (|m4| / m2^2 + 3))

(1.01: the second-order terms, given dm2 / m2 < 1e-4, which `reference` asserts).  Mean and variance, in the units of x with
h = (hi - lo) / 2:  tol_mean = h da1 + 4 eps (|c| + h |a1|),  tol_var = 1.01 h^2 (dm2 + 8 eps m2) N / (N - 1).
A coordinate with a NaN or an inf among its draws has non-finite sums, moments and bounds.
"""
import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble


def columns(x, lo, hi, B):
    """The column of every draw: x [..., p] -> int64 [..., p]."""
    x = np.asarray(x, dtype=np.float64)
    invw = B / (hi - lo)
    with np.errstate(invalid="ignore"):
        t = (x - lo) * invw
        inside = (t >= 0) & (t < B)
        col = 1 + np.floor(np.where(inside, t, 0.0)).astype(np.int64)
        col = np.where((t >= B) | (x >= hi), B + 1, col)
        col = np.where(t < 0, 0, col)
    return np.where(np.isnan(x), B + 2, col)


def reference(x, lo, hi, B):
    """x [n, C, p] float64 (already rounded to the dtype under test) -> dict: counts [p, B + 3] uint64, table [6, p], tol_table [6, p] (rows 0,
    1: 0), mean, variance, skewness, kurtosis, tol_mean, tol_variance, tol_skewness, tol_kurtosis [p], finite [p] bool."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n, C, p = x.shape
    N = n * C
    X = x.reshape(N, p)
    col = columns(X, lo, hi, B)
    counts = np.zeros((p, B + 3), dtype=np.uint64)
    for j in range(p):
        counts[j] = np.bincount(col[:, j], minlength=B + 3)
    table = np.full((6, p), np.nan)
    tol = np.zeros((6, p))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        some = ~np.all(np.isnan(X), axis=0)
        table[0, some] = np.nanmin(X[:, some], axis=0)
        table[1, some] = np.nanmax(X[:, some], axis=0)
        c, s = (lo + hi) / 2.0, 2.0 / (hi - lo)
        u = ((X - c) * s).astype(LD)  # float64 operations, as the header spells them; the powers and sums below in long double
        S = np.stack([(u ** k).sum(axis=0) for k in (1, 2, 3, 4)])
        A = np.stack([(np.abs(u) ** k).sum(axis=0) for k in (1, 2, 3, 4)])
        finite = np.all(np.isfinite(X), axis=0)
        table[2:] = S.astype(np.float64)
        tol[2:] = ((N + 4) * LD(EPS) * A).astype(np.float64)
        # two passes over the draws themselves
        L = X.astype(LD)
        mean = L.sum(axis=0) / N
        d = L - mean
        M2, M3, M4 = (d ** 2).sum(axis=0) / N, (d ** 3).sum(axis=0) / N, (d ** 4).sum(axis=0) / N
        variance = M2 * N / (N - 1) if N > 1 else np.full(p, np.nan, dtype=LD)
        skew, kurt = M3 / M2 ** LD(1.5), M4 / (M2 * M2) - 3
        # the bounds, from the power sums of u
        e = LD(EPS)
        k = np.arange(1, 5, dtype=LD)[:, None]
        E = (N + 4) * e * A + 2 * k * e * A
        a = S / N
        da = E / N + e * np.abs(a)
        a1, a2, a3, a4 = a
        d1, d2, d3, d4 = da
        m2 = a2 - a1 * a1
        m3 = a3 - 3 * a1 * a2 + 2 * a1 ** 3
        m4 = a4 - 4 * a1 * a3 + 6 * a1 * a1 * a2 - 3 * a1 ** 4
        dm2 = d2 + 2 * abs(a1) * d1 + 3 * e * (abs(a2) + a1 * a1)
        dm3 = d3 + 3 * (abs(a2) * d1 + abs(a1) * d2) + 6 * a1 * a1 * d1 + 4 * e * (abs(a3) + 3 * abs(a1 * a2) + 2 * abs(a1) ** 3)
        dm4 = (d4 + 4 * (abs(a3) * d1 + abs(a1) * d3) + 6 * (2 * abs(a1 * a2) * d1 + a1 * a1 * d2) + 12 * abs(a1) ** 3 * d1
               + 5 * e * (abs(a4) + 4 * abs(a1 * a3) + 6 * a1 * a1 * abs(a2) + 3 * a1 ** 4))
        tol_skew = LD(1.01) * (dm3 / m2 ** LD(1.5) + LD(1.5) * abs(m3) * dm2 / m2 ** LD(2.5) + 4 * e * abs(m3 / m2 ** LD(1.5)))
        tol_kurt = LD(1.01) * (dm4 / (m2 * m2) + 2 * abs(m4) * dm2 / m2 ** 3 + 4 * e * (abs(m4) / (m2 * m2) + 3))
        h = (hi - lo) / 2.0
        tol_mean = h * d1 + 4 * e * (np.abs(c) + h * abs(a1))
        tol_var = LD(1.01) * h * h * (dm2 + 8 * e * m2) * N / (N - 1) if N > 1 else np.full(p, np.nan, dtype=LD)
        shaped = finite & (np.asarray(M2, dtype=np.float64) > 0)  # skewness and kurtosis exist
        assert np.all(np.asarray(dm2 / m2, dtype=np.float64)[shaped] < 1e-4)
    f64 = lambda v, ok: np.where(ok, np.asarray(v, dtype=np.float64), np.nan)  # noqa: E731
    return {"n": n, "C": C, "B": B, "counts": counts, "table": table, "tol_table": tol, "finite": finite, "shaped": shaped,
            "mean": f64(mean, finite), "variance": f64(variance, finite), "skewness": f64(skew, shaped), "kurtosis": f64(kurt, shaped),
            "tol_mean": f64(tol_mean, finite), "tol_variance": f64(tol_var, finite), "tol_skewness": f64(tol_skew, shaped),
            "tol_kurtosis": f64(tol_kurt, shaped)}


def compare(counts, table, res, ref):
    """-> (largest error / bound over rows 2..5 of the table and over mean, variance, skewness, kurtosis of `res`; list of complaints).
    Counts and min / max must agree exactly; a sum or a moment is finite exactly where the reference's is."""
    bad = []
    counts, table = np.asarray(counts), np.asarray(table)
    if counts.shape != ref["counts"].shape or table.shape != ref["table"].shape:
        return np.inf, [f"shapes {counts.shape} {table.shape}"]
    if counts.dtype != np.uint64 or not np.array_equal(counts, ref["counts"]):
        bad.append(f"counts differ in {int(np.sum(counts != ref['counts']))} cells")
    if not np.array_equal(table[:2], ref["table"][:2], equal_nan=True):
        bad.append(f"min / max {table[:2].tolist()} != {ref['table'][:2].tolist()}")
    worst = 0.0
    pairs = [(f"S{k + 1}", table[2 + k], ref["table"][2 + k], ref["tol_table"][2 + k]) for k in range(4)]
    if res is not None:
        pairs += [(key, np.asarray(res[key]), ref[key], ref["tol_" + key]) for key in ("mean", "variance", "skewness", "kurtosis")]
    for name, got, want, tol in pairs:
        if not np.array_equal(np.isfinite(got), np.isfinite(want)):
            bad.append(f"{name}: finite at {np.isfinite(got).tolist()}, reference {np.isfinite(want).tolist()}")
            continue
        ok = np.isfinite(want)
        if not ok.any():
            continue
        err, t = np.abs(got[ok] - want[ok]), tol[ok]
        exact = t == 0
        if np.any(err[exact] != 0):
            bad.append(f"{name}: entries with bound 0 differ (largest {err[exact].max():.3e})")
        if np.any(~exact):
            ratio = float(np.max(err[~exact] / t[~exact]))
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append(f"{name}: error / bound = {ratio:.3e}")
    return worst, bad
