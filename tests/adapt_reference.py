"""TEST INFRASTRUCTURE: the definition of include/logreg_hip_adapt.h restated in NumPy, independent of the kernels -- the schedule, dual
averaging in float64, the pooled window variance in np.longdouble straight from the draws (two passes, no Chan merge), and the error
bounds of the device's float64 arithmetic derived from the inputs alone (in the manner of marginals_reference.py / cov_reference.py).

Bounds (u = 2^-53, the unit roundoff of float64):
    abar_t   the device adds C non-negative float64 numbers in a fixed tree and divides once: |err| <= (C + 4) u sum|a| / C.
    M2       the device's M2 is a sum of non-negative terms (squares about workgroup means, Chan's between-group terms), each formed with a
             few roundings, added along paths no longer than the N pooled values: (N + 4) u M2 for the sums; every mean it subtracts
             carries an error of at most dm = (N + 4) u max|x| (a sum of <= N values of size <= max|x|, one division), and moving the
             means of a decomposition sum_b n_b (mean_b - mean)^2 + within by dm changes it by at most 2 dm sqrt(N M2) + 2 N dm^2
             (Cauchy-Schwarz on sum n_b |mean_b - mean|).     tol_M2 = (N + 4) u M2 + 2 dm sqrt(N M2) + 2 N dm^2
    var, inv_metric, dmm   propagated: one division, a product, a sum, a reciprocal -- 2 u, 4 u, 2 u relative on top.
"""
import numpy as np

U = 2.0 ** -53
DEFAULTS = dict(delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, eps0=1.0)


def schedule(W, init=75, term=50, base=25):
    """-> (first iteration of the first window or W, [exclusive window ends])"""
    W, init, term, base = int(W), int(init), int(term), int(base)
    if W < 20:
        return W, []
    if init + base + term > W:
        init = int(np.floor(0.15 * W))
        term = int(np.floor(0.10 * W))
        base = W - init - term
    ends, start, size = [], init, base
    while start < W - term and size > 0:
        end = start + size
        if end + 2 * size > W - term:
            end = W - term
        ends.append(end)
        start, size = end, 2 * size
    return (init if ends else W), ends


def windows_of(W, init, ends):
    """-> window index per iteration (-1 outside), [last iteration of each window]"""
    idx = np.full(W, -1, dtype=np.int64)
    start = init
    for k, e in enumerate(ends):
        idx[start:e] = k
        start = e
    return idx, [e - 1 for e in ends]


def dual_averaging(abar, restarts=(), eps0=1.0, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, m_offset=0, keep_hbar=False):
    """The step-size recursion of the header on a sequence abar[t] in float64.  restarts: iterations after whose update dual averaging
    restarts from the step just computed.  -> dict(eps [W]: the step iteration t USES, log_eps_bar [W]: after iteration t's step, final).
    m_offset, keep_hbar: the mutations of tests/test_adapt_cpu.py (m off by one; a restart that keeps Hbar)."""
    abar = np.asarray(abar, dtype=np.float64)
    W = len(abar)
    eps_used, leb = np.empty(W), np.empty(W)
    eps = np.float64(eps0)
    mu, hbar, log_eps_bar, m = np.log(np.float64(10.0) * eps), np.float64(0.0), np.float64(0.0), 0
    restarts = set(int(r) for r in restarts)
    for t in range(W):
        eps_used[t] = eps
        m += 1
        mm = np.float64(m + m_offset)
        hbar = (np.float64(1.0) - np.float64(1.0) / (mm + t0)) * hbar + (np.float64(delta) - abar[t]) / (mm + t0)
        log_eps = mu - np.sqrt(mm) / np.float64(gamma) * hbar
        eta = np.power(mm, -np.float64(kappa))
        log_eps_bar = eta * log_eps + (np.float64(1.0) - eta) * log_eps_bar
        eps = np.exp(log_eps)
        leb[t] = log_eps_bar
        if t in restarts:
            mu = np.log(np.float64(10.0) * eps)
            log_eps_bar, m = np.float64(0.0), 0
            if not keep_hbar:
                hbar = np.float64(0.0)
    return {"eps": eps_used, "log_eps_bar": leb, "final": float(np.exp(leb[-1])), "next": float(eps)}


def abar_of(astat):
    """astat [W, C] float64 -> (abar [W] rounded from np.longdouble, tol [W])"""
    a = np.asarray(astat, dtype=np.float64)
    C = a.shape[1]
    s = a.astype(np.longdouble).sum(axis=1)
    return (s / C).astype(np.float64), (C + 4) * U * np.abs(a).sum(axis=1) / C + U  # (+ u: the reference's own rounding to float64)


def metric_of(x, dmm_before):
    """One window: x [L, C, p] (any float dtype; converted exactly) -> dict(n, var, dmm, skipped [p] bool, tol_var, tol_dmm)."""
    xl = np.asarray(x).astype(np.longdouble).reshape(-1, np.shape(x)[-1])
    N = xl.shape[0]
    with np.errstate(all="ignore"):
        mean = xl.sum(axis=0) / N
        M2 = ((xl - mean) ** 2).sum(axis=0)
        var = M2 / (N - 1) if N > 1 else np.full(xl.shape[1], np.nan, dtype=np.longdouble)
        ok = np.isfinite(var) & (var > 0)
        a, c = np.longdouble(N) / (N + 5), np.longdouble(1e-3) * 5 / (N + 5)
        inv = a * var + c
        dmm = np.where(ok, 1 / np.where(ok, inv, 1), np.asarray(dmm_before, dtype=np.longdouble))
        xmax = np.max(np.abs(np.where(np.isfinite(xl), xl, 0)), axis=0)
        dm = (N + 4) * U * xmax
        tol_M2 = (N + 4) * U * M2 + 2 * dm * np.sqrt(N * M2) + 2 * N * dm * dm
        tol_var = tol_M2 / max(N - 1, 1) + 2 * U * np.abs(var)
        tol_inv = a * tol_var + 4 * U * np.abs(inv)
        tol_dmm = np.where(ok, tol_inv / np.where(ok, inv, 1) ** 2 + 2 * U * np.abs(dmm), 0)
    return {"n": N, "var": var.astype(np.float64), "dmm": dmm.astype(np.float64), "skipped": ~ok, "tol_var": tol_var.astype(np.float64) + U * np.abs(var.astype(np.float64)),
            "tol_dmm": tol_dmm.astype(np.float64) + U * np.abs(dmm.astype(np.float64))}


def teacher_forced(astat, draws, W, dmm0, adapt_metric=True, buffers=(75, 50, 25), **da):
    """The whole adaptation recomputed from the device's own acceptance statistics astat [W, C] and states draws [W, C, p].
    -> dict(abar, tol_abar, eps, log_eps_bar, final, window [W], n [W], metric: [dict per window], dmm, skipped)"""
    astat = np.asarray(astat, dtype=np.float64)
    C = astat.shape[1]
    init, ends = schedule(W, *buffers)
    if not adapt_metric:
        init, ends = W, []
    idx, lasts = windows_of(W, init, ends)
    abar, tol = abar_of(astat)
    opts = dict(DEFAULTS)
    opts.update(da)
    d = dual_averaging(abar, lasts, **opts)
    dmm = np.array(np.broadcast_to(np.asarray(dmm0, dtype=np.float64), (np.shape(draws)[-1],)))
    metric, start, skipped = [], init, 0
    for e in ends:
        mt = metric_of(np.asarray(draws)[start:e], dmm)
        dmm = mt["dmm"]
        skipped += int(mt["skipped"].sum())
        metric.append(mt)
        start = e
    n = np.zeros(W)
    start = init
    for e in ends:
        n[start:e] = C * (np.arange(start, e) - start + 1)
        start = e
    return {"abar": abar, "tol_abar": tol, "eps": d["eps"], "log_eps_bar": d["log_eps_bar"], "final": d["final"], "window": idx, "n": n,
            "metric": metric, "dmm": dmm, "skipped": skipped}
