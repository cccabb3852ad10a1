"""include/logreg_hip_rank.h restated in float64 NumPy, line by line: the yardstick of tests/test_rank_cpu.py and tests/test_gpu_rank.py.

Nothing here shares code with the library: ranks come from np.sort + np.searchsorted on the widened draws, the inverse normal CDF is
AS 241 typed in again (and checked against scipy.special.ndtri in tests/test_rank_cpu.py), the autocovariances are plain dot products.
"""
import numpy as np

ROWS = ("rhat_bulk", "rhat_tail", "rhat", "ess_bulk", "ess_tail", "capped_bulk", "capped_q05", "capped_q95", "median", "q05", "q95", "n_nonfinite",
        "pairs_bulk", "pairs_q05", "pairs_q95")

_A = [3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4, 4.5921953931549871457e4,
      6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3]
_B = [1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4, 3.9307895800092710610e4,
      2.8729085735721942674e4, 5.2264952788528545610e3]
_C = [1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504, 1.27045825245236838258,
      2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4]
_D = [1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1, 1.48103976427480074590e-1, 1.51986665636164571966e-2,
      5.47593808499534494600e-4, 1.05075007164441684324e-9]
_E = [6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1, 2.65321895265761230930e-2,
      1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7]
_F = [1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4, 1.84631831751005468180e-5,
      1.42151175831644588870e-7, 2.04426310338993978564e-15]


def _poly(c, r):
    out = np.full_like(r, c[-1])
    for a in c[-2::-1]:
        out = out * r + a
    return out


def ndtri(p):
    """Wichura's AS 241 (PPND16), vectorised"""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * _poly(_A, r) / _poly(_B, r)
    t = ~mid
    r = np.sqrt(-np.log(np.where(q[t] < 0.0, p[t], 1.0 - p[t])))
    near = r <= 5.0
    v = np.empty_like(r)
    v[near] = _poly(_C, r[near] - 1.6) / _poly(_D, r[near] - 1.6)
    v[~near] = _poly(_E, r[~near] - 5.0) / _poly(_F, r[~near] - 5.0)
    out[t] = np.where(q[t] < 0.0, -v, v)
    return out


def twice_ranks(x):
    """2r = lo + hi + 1 of every entry of x (any shape) among all of them, int64; -0.0 ties with +0.0"""
    x = np.asarray(x, dtype=np.float64)
    flat = x.ravel() + 0.0  # (-0.0 + 0.0 = +0.0)
    s = np.sort(flat)
    lo = np.searchsorted(s, flat, side="left")
    hi = np.searchsorted(s, flat, side="right")
    return (lo + hi + 1).astype(np.int64).reshape(x.shape)


def z_of(twice_r, S):
    return ndtri((np.asarray(twice_r, dtype=np.float64) * 0.5 - 0.375) / (S + 0.25))


def used(x):
    """x [n, C] -> the 2h used steps, h"""
    h = x.shape[0] // 2
    return np.asarray(x[:2 * h], dtype=np.float64), h


def split(v, h):
    """v [2h, C] -> [h, M] with split chain m = 2c + (t >= h)"""
    C = v.shape[1]
    out = np.empty((h, 2 * C))
    out[:, 0::2] = v[:h]
    out[:, 1::2] = v[h:2 * h]
    return out


def order_stats(x2):
    """x2 [2h, C] -> med, q05, q95"""
    s = np.sort(x2.ravel() + 0.0)
    S = s.size
    return (s[S // 2 - 1] + s[S // 2]) * 0.5, s[(S - 1) // 20], s[19 * (S - 1) // 20]


def chain_moments(v, max_lag):
    """v [h, M] -> mean_m [M], acov [L + 1, M], L = min(max_lag, h - 1), pivoted at each chain's first value"""
    h = v.shape[0]
    L = min(max_lag, h - 1)
    d = v - v[0]
    dbar = d.sum(axis=0) / h
    e = d - dbar
    acov = np.stack([np.einsum("tm,tm->m", e[:h - l], e[l:]) / h for l in range(L + 1)])
    return v[0] + dbar, acov


def w_v(v, max_lag):
    h, M = v.shape
    mean, acov = chain_moments(v, max_lag)
    W = acov[0].sum() / M * h / (h - 1.0)
    d = mean - mean[0]
    B = (np.sum(d * d) - d.sum() ** 2 / M) / (M - 1.0)
    return W, (h - 1.0) / h * W + B, acov


def rhat(v):
    """step 5 on v [h, M]"""
    if v.shape[0] < 2:
        return np.nan
    W, V, _ = w_v(v, 0)
    return np.sqrt(V / W) if W > 0.0 and np.isfinite(V) else np.nan


def ess(v, max_lag):
    """step 6 on v [h, M] -> dict(ess, capped, pairs, margin = |the pair that ended the scan| (inf if none did))"""
    h, M = v.shape
    nan = dict(ess=np.nan, capped=np.nan, pairs=np.nan, margin=np.inf)
    if h < 2:
        return nan
    S = h * M
    L = min(max_lag, h - 1)
    W, V, acov = w_v(v, max_lag)
    if not (W > 0.0 and np.isfinite(V)):
        return nan
    rho = 1.0 - (W - acov.sum(axis=1) / M) / V
    rho[0] = 1.0
    total, prev, last, k, stopped, margin = 0.0, 0.0, 0.0, 0, False, np.inf
    for k in range((L + 1) // 2 + 1):
        if k == (L + 1) // 2:
            break
        P = rho[2 * k] + rho[2 * k + 1]
        if not P > 0.0:
            stopped, last, margin = True, max(rho[2 * k], 0.0), abs(P)
            break
        margin = min(margin, abs(P))  # (a kept pair near zero is as fragile as the one that ends the scan)
        if k > 0:
            P = min(P, prev)
        total += P
        prev = P
    tau = max(-1.0 + 2.0 * total + last, 1.0 / np.log10(S))
    return dict(ess=S / tau, capped=float(not stopped and L == max_lag and h - 1 > max_lag), pairs=float(k), margin=margin)


def column(x, max_lag, z=None, zf=None):
    """One coordinate x [n, C] -> dict of the header's rows (+ twice_r, twice_rf [2h, C], z, zf, margin).  z, zf [2h, C]: use these
    z-scales in place of the reference's own (the statistics of the device's z)."""
    x2, h = used(x)
    S = x2.size
    out = {k: np.nan for k in ROWS}
    out["n_nonfinite"] = int(np.sum(~np.isfinite(x2))) if h >= 2 else 0
    out["margin"] = np.inf
    if h < 2 or out["n_nonfinite"]:
        return out
    med, q05, q95 = order_stats(x2)
    r2 = twice_ranks(x2)
    r2f = twice_ranks(np.abs(x2 - med))
    zz = z_of(r2, S) if z is None else np.asarray(z, dtype=np.float64)
    zzf = z_of(r2f, S) if zf is None else np.asarray(zf, dtype=np.float64)
    out.update(median=med, q05=q05, q95=q95, twice_r=r2, twice_rf=r2f, z=zz, zf=zzf)
    out["rhat_bulk"], out["rhat_tail"] = rhat(split(zz, h)), rhat(split(zzf, h))
    out["rhat"] = max(out["rhat_bulk"], out["rhat_tail"]) if not (np.isnan(out["rhat_bulk"]) or np.isnan(out["rhat_tail"])) else np.nan
    eb = ess(split(zz, h), max_lag)
    e05 = ess(split((x2 <= q05).astype(np.float64), h), max_lag)
    e95 = ess(split((x2 <= q95).astype(np.float64), h), max_lag)
    out.update(ess_bulk=eb["ess"], capped_bulk=eb["capped"], pairs_bulk=eb["pairs"], capped_q05=e05["capped"], pairs_q05=e05["pairs"],
               capped_q95=e95["capped"], pairs_q95=e95["pairs"])
    out["ess_tail"] = min(e05["ess"], e95["ess"]) if not (np.isnan(e05["ess"]) or np.isnan(e95["ess"])) else np.nan
    out["margin"] = min(eb["margin"], e05["margin"], e95["margin"])
    return out


def table(x, max_lag=63, z=None, zf=None):
    """x [n, C, p] -> (table [15, p] as lr_rank_result gives it, margin [p]); z, zf: lists per coordinate as in `column`"""
    x = np.asarray(x)
    p = x.shape[2]
    T = np.full((len(ROWS), p), np.nan)
    margin = np.full(p, np.inf)
    for j in range(p):
        c = column(x[:, :, j], max_lag, None if z is None else z[j], None if zf is None else zf[j])
        T[:, j] = [c[k] for k in ROWS]
        margin[j] = c["margin"]
    return T, margin


def classical_split_rhat(x):
    """the mean / variance split-R-hat of one coordinate x [n, C] (diagnostics.split_rhat's definition)"""
    x2, h = used(x)
    return rhat(split(x2, h))


def ar1(rng, n, C, phi):
    """C stationary AR(1) chains of n steps with unit innovation variance"""
    x = np.empty((n, C))
    x[0] = rng.standard_normal(C) / np.sqrt(1.0 - phi * phi)
    eps = rng.standard_normal((n, C))
    for t in range(1, n):
        x[t] = phi * x[t - 1] + eps[t]
    return x
