"""A plain NumPy reference of the horseshoe Polya-Gamma Gibbs sampler -- TEST INFRASTRUCTURE ONLY (a helper module, imported by the
horseshoe tests).

Written from the text of include/logreg_hip_hs.h on top of tests/pg_reference.py (its Philox, its draw of omega, its normals).  It shares
no arithmetic with the kernel (logreg_amd/csrc/lr_hs.h) or the CPU test double (tests/host/lr_cpu_twin_hs.c): the hyper-step runs on
whole arrays over chains and coordinates, its sums are numpy.sum, and the beta-step factorises the unscaled matrix of every chain with
numpy.linalg.cholesky, as pg_reference.sweep does.

Also here: the small model of the target check (`small_model`) and the statistics the posterior tests compare with
tests/golden/hs_small_posterior.json (`posterior_quantities`, `z_against_fixture`).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pg_reference as pr

TAG = 0x02000000  # LR_HS_TAG
BLOCK_GLOBAL, BLOCK_GAMMA = 32, 33
LO, HI = 1e-100, 1e100
# |z| below which every stored quantity of the small model must lie: the suite's family-wise bound (tests/test_gpu_pg.py)
Z_BOUND = 4.2


def expo(wa, wb):
    """E = -ln u53(wa, wb)"""
    u = (((wa >> np.uint64(5)).astype(np.float64) * 67108864.0 + (wb >> np.uint64(6)).astype(np.float64)) + 0.5) * 2.0 ** -53
    return -np.log(u)


def _clamp(new, old):
    """step 7 -> (values, 1 where a clamp happened)"""
    nan = np.isnan(new)
    with np.errstate(invalid="ignore"):
        lo, hi = new < LO, new > HI
    out = np.where(nan, old, np.where(lo, LO, np.where(hi, HI, new)))
    return out, (nan | lo | hi).astype(np.int64)


def default_hyper(C, p, tau0):
    h = np.ones((C, 2 * p + 2))
    h[:, 2 * p] = tau0 * tau0
    return h


def hyper_step(beta, hyper, mask, tau0, seed, chains, it):
    """steps 5-7 of include/logreg_hip_hs.h for every chain: beta [C, p] (the new state as stored), hyper [C, 2p+2] -> (new hyper, clamped [C])"""
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    C, p = beta.shape
    hyper = np.asarray(hyper, dtype=np.float64).reshape(C, 2 * p + 2)
    mask = np.asarray(mask, dtype=bool)
    chains = np.asarray(chains, dtype=np.uint64)
    lo, hi = int(it) & 0xFFFFFFFF, (int(it) >> 32) & 0xFFFFFFFF
    lam, nu, tau2, xi = hyper[:, :p], hyper[:, p:2 * p], hyper[:, 2 * p], hyper[:, 2 * p + 1]
    with np.errstate(all="ignore"):
        w = pr.philox(chains[:, None], lo, hi, np.uint64(TAG) | np.arange(p, dtype=np.uint64)[None, :], seed, int(seed) >> 32)
        b2 = beta * beta
        lam_new, c1 = _clamp((1.0 / nu + b2 * (0.5 * (1.0 / tau2))[:, None]) / expo(w[0], w[1]), lam)
        nu_new, c2 = _clamp((1.0 + 1.0 / lam_new) / expo(w[2], w[3]), nu)
        lam_new, nu_new = np.where(mask, lam_new, lam), np.where(mask, nu_new, nu)
        clamped = ((c1 + c2) * mask).sum(axis=1)
        quad = np.where(mask, b2 * (1.0 / lam_new), 0.0).sum(axis=1)
        m = int(mask.sum())
        nexp = (m + 1) // 2
        k = np.arange(16, dtype=np.uint64)
        wg = pr.philox(chains[:, None], lo, hi, np.uint64(TAG) | (np.uint64(BLOCK_GAMMA) + (k >> np.uint64(1)))[None, :], seed, int(seed) >> 32)
        e = np.where((k & np.uint64(1)).astype(bool)[None, :], expo(wg[2], wg[3]), expo(wg[0], wg[1]))
        g = e[:, :nexp].sum(axis=1)
        w3 = pr.philox(chains, lo, hi, TAG | BLOCK_GLOBAL, seed, int(seed) >> 32)
        if (m + 1) & 1:
            z = np.sqrt(-2.0 * np.log((w3[2].astype(np.float64) + 0.5) * 2.0 ** -32)) * np.cos(2.0 * np.pi * ((w3[3].astype(np.float64) + 0.5) * 2.0 ** -32))
            g = g + 0.5 * z * z
        tau_new, c3 = _clamp((1.0 / xi + 0.5 * quad) / g, tau2)
        xi_new, c4 = _clamp((1.0 / (tau0 * tau0) + 1.0 / tau_new) / expo(w3[0], w3[1]), xi)
    return np.concatenate([lam_new, nu_new, tau_new[:, None], xi_new[:, None]], axis=1), clamped + c3 + c4


@dataclass
class Sweep:
    beta: np.ndarray       # [C, p] the new states (the model's dtype)
    hyper: np.ndarray      # [C, 2p+2]
    margin: np.ndarray     # [C, n] decision margins of the omega draws
    proposals: np.ndarray  # [C]
    terms: np.ndarray
    skipped: np.ndarray    # [C] bool
    clamped: np.ndarray    # [C]


def _sanitise(hyper):
    h = np.asarray(hyper, dtype=np.float64)
    return np.where(np.isnan(h), 1.0, np.clip(h, LO, HI))


def sweep(Xs, pscale, beta, hyper, mask, tau0, seed, chains, it, dtype=np.float64) -> Sweep:
    """one iteration of every chain: Xs [n, p] signed rows, beta [C, p], hyper [C, 2p+2], chains [C] global chain ids"""
    dt = np.dtype(dtype).type
    Xs = np.ascontiguousarray(Xs, dtype=dt)
    beta = np.atleast_2d(np.asarray(beta, dtype=dt))
    C, p = beta.shape
    n = Xs.shape[0]
    hyper = _sanitise(hyper).reshape(C, 2 * p + 2)
    mask = np.asarray(mask, dtype=bool)
    chains = np.asarray(chains, dtype=np.uint64)
    with np.errstate(all="ignore"):
        psi = (beta @ Xs.T).astype(dt)
    fin = np.isfinite(psi)
    d = pr.draw(np.where(fin, psi, dt(0)), seed, chains[:, None], it, np.arange(n, dtype=np.uint64)[None, :], dtype)
    skipped = ~fin.all(axis=1)
    X64 = Xs.astype(np.float64)
    b = 0.5 * X64.sum(axis=0)
    ivar = 1.0 / np.broadcast_to(np.asarray(pscale, dtype=np.float64), (p,)) ** 2
    prec = ivar[None, :] + mask[None, :] * ((1.0 / hyper[:, 2 * p])[:, None] * (1.0 / hyper[:, :p]))
    z = pr.normals(seed, chains, it, p)
    A = np.einsum("cn,nj,nk->cjk", d["omega"].astype(np.float64), X64, X64)
    A[:, np.arange(p), np.arange(p)] += prec
    new = beta.astype(np.float64).copy()
    for c in range(C):
        if skipped[c]:
            continue
        try:
            L = np.linalg.cholesky(A[c])
        except np.linalg.LinAlgError:
            skipped[c] = True
            continue
        mean = np.linalg.solve(L.T, np.linalg.solve(L, b))
        new[c] = mean + np.linalg.solve(L.T, z[c])
    new = new.astype(dt)
    live = ~skipped
    h_new, clamped = hyper_step(new.astype(np.float64), hyper, mask, tau0, seed, chains, it)
    h_new = np.where(live[:, None], h_new, hyper)
    return Sweep(new, h_new, d["margin"], np.where(live, d["proposals"].sum(axis=1), 0), np.where(live, d["terms"].sum(axis=1), 0), skipped, np.where(live, clamped, 0))


def run_small(Xs, pscale, beta, hyper, mask, tau0, seed, iters, drop=0):
    """the float64 sampler on a model small enough for closed 3 x 3 algebra on whole arrays of chains (no Python loop over chains):
    -> (beta [iters, C, p], lambda^2 [iters, C, p], tau^2 [iters, C]) of the sweeps after the first `drop`"""
    Xs = np.asarray(Xs, dtype=np.float64)
    beta = np.array(beta, dtype=np.float64)
    C, p = beta.shape
    n = Xs.shape[0]
    hyper = np.array(hyper, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    chains = np.arange(C, dtype=np.uint64)
    b = 0.5 * Xs.sum(axis=0)
    ivar = 1.0 / np.asarray(pscale, dtype=np.float64) ** 2
    kept_b, kept_l, kept_t = [], [], []
    for it in range(drop + iters):
        psi = beta @ Xs.T
        om = pr.draw(psi, seed, chains[:, None], it, np.arange(n, dtype=np.uint64)[None, :])["omega"]
        A = np.einsum("cn,nj,nk->cjk", om, Xs, Xs)
        A[:, np.arange(p), np.arange(p)] += ivar[None, :] + mask[None, :] * ((1.0 / hyper[:, 2 * p])[:, None] * (1.0 / hyper[:, :p]))
        L = np.linalg.cholesky(A)
        Lt = np.swapaxes(L, 1, 2)
        z = pr.normals(seed, chains, it, p)
        y = np.linalg.solve(L, np.broadcast_to(b, (C, p))[:, :, None])
        beta = np.linalg.solve(Lt, y + z[:, :, None])[:, :, 0]
        hyper, _ = hyper_step(beta, hyper, mask, tau0, seed, chains, it)
        if it >= drop:
            kept_b.append(beta.copy())
            kept_l.append(hyper[:, :p].copy())
            kept_t.append(hyper[:, 2 * p].copy())
    return np.array(kept_b), np.array(kept_l), np.array(kept_t)


# ---- the small model of the target check (include/logreg_hip_hs.h "The model"): n = 12, p = 3, coordinate 0 unshrunk
SMALL_PSCALE = np.array([3.0, 2.0, 2.0])
SMALL_MASK = np.array([False, True, True])
SMALL_TAU0 = 1.0


def small_model():
    """-> (X [12, 3], y [12]) from a seeded generator: an intercept, two standard-normal covariates, labels from beta = (0.3, 1.5, 0)"""
    rng = np.random.default_rng(20240611)
    X = rng.standard_normal((12, 3))
    X[:, 0] = 1.0
    y = (rng.random(12) < 1.0 / (1.0 + np.exp(-X @ np.array([0.3, 1.5, 0.0])))).astype(np.float64)
    return X, y


def posterior_quantities(beta, lam2, tau2, mask=SMALL_MASK):
    """the draws of the stored quantities, [iters, C, q]: beta_j (all j), kappa_j = 1 / (1 + tau^2 lambda_j^2) for j in S, log tau^2"""
    beta, lam2, tau2 = (np.asarray(a, dtype=np.float64) for a in (beta, lam2, tau2))
    kappa = 1.0 / (1.0 + tau2[..., None] * lam2[..., mask])
    return np.concatenate([beta, kappa, np.log(tau2)[..., None]], axis=-1)


def z_against_fixture(q, fixture, summarise):
    """z of every stored quantity: the means of all q columns and the sd of the beta columns, with the MCSE combined from
    summarise(max_chains=128) and the fixture's -> (z of the means [q], z of the sds [p])"""
    s = summarise(q, max_chains=128)
    mean, mcse = np.array(fixture["mean"]), np.array(fixture["mean_mcse"])
    zm = (s["mean"] - mean) / np.sqrt(s["mcse"] ** 2 + mcse ** 2)
    p = len(fixture["sd"])
    se_sd = s["sd"][:p] / np.sqrt(2 * s["ess"][:p])
    zs = (s["sd"][:p] - np.array(fixture["sd"])) / np.sqrt(se_sd ** 2 + np.array(fixture["sd_mcse"]) ** 2)
    return zm, zs


# ---- hyper-states for the tests of lr_hs_hyper: log-uniform over 10^+-6, one chain at the clamp
def random_hyper(rng, C, p):
    h = 10.0 ** rng.uniform(-6.0, 6.0, (C, 2 * p + 2))
    h[0, :] = np.where(np.arange(2 * p + 2) % 2 == 0, LO, HI)  # 1 / nu = 1e100 and friends: the new values leave the range
    return h


def random_mask(rng, p):
    m = rng.random(p) < 0.7
    m[0] = False
    m[p - 1] = True
    return m


def hyper_dev(a, b):
    """largest elementwise relative deviation of two hyper-states"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- one call of the C ABI of whatever library is loaded (the device library, the second build or the CPU double) on a pg_reference case
def _prior(mask, tau0):
    from logreg_amd import _lib
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    return m8, _lib.HsPrior(m8.ctypes.data, float(tau0))


def _opts(case, iters=1):
    from logreg_amd import _lib
    return _lib.RunOpts(n_chains=case.C, chain_offset=case.chain_offset, thin=1, iters=iters, iter_offset=case.iter_offset, seed=case.seed, group=0,
                        mode=_lib.MODE_AUTO, on_device=0)


def library_hyper(la, case, dtype, mask, tau0, hyper, states=None):
    """lr_hs_hyper on the case -> (hyper_out [C, 2p+2], clamped [C])"""
    import ctypes
    from logreg_amd import _lib
    L = _lib.load_hs()
    X, y, ps, st = pr.make_case(case)
    m = la.LogReg(X, y, ps, dtype=dtype)
    st = np.ascontiguousarray(st if states is None else states, dtype=m.np_dtype)
    hin = np.ascontiguousarray(hyper, dtype=np.float64)
    before_s, before_h = st.tobytes(), hin.tobytes()
    hout = np.full_like(hin, np.nan)
    cn = np.zeros(case.C, dtype=la.kernels.HS_COUNTERS)
    keep, prior = _prior(mask, tau0)
    opts = _opts(case)
    assert L.lr_hs_hyper(m.handle, ctypes.byref(prior), st.ctypes.data, hin.ctypes.data, ctypes.byref(opts), hout.ctypes.data, cn.ctypes.data) == 0, L.lr_last_error()
    assert st.tobytes() == before_s and hin.tobytes() == before_h  # nothing is moved
    assert not cn["proposals"].any() and not cn["series_terms"].any() and not cn["skipped"].any()
    m.close()
    return hout, cn["clamped"].astype(np.int64)


def library_sweep(la, case, dtype, mask, tau0, hyper, states=None):
    """one sweep of lr_run_hs on the case -> (new states [C, p], new hyper [C, 2p+2], counters [C])"""
    import ctypes
    from logreg_amd import _lib
    L = _lib.load_hs()
    X, y, ps, st = pr.make_case(case)
    m = la.LogReg(X, y, ps, dtype=dtype)
    st = np.ascontiguousarray(st if states is None else states, dtype=m.np_dtype).copy()
    h = np.ascontiguousarray(hyper, dtype=np.float64).copy()
    cn = np.zeros(case.C, dtype=la.kernels.HS_COUNTERS)
    keep, prior = _prior(mask, tau0)
    opts = _opts(case)
    assert L.lr_run_hs(m.handle, ctypes.byref(prior), st.ctypes.data, h.ctypes.data, ctypes.byref(opts), None, None, cn.ctypes.data) == 0, L.lr_last_error()
    m.close()
    return st, h, cn


def case_prior(case):
    """-> (mask [p], tau0, hyper [C, 2p+2]) of a pg_reference case: a random mask without coordinate 0, scales log-uniform over 10^+-2 (the
    sweep's own range: the posterior's), seeded by the case"""
    rng = np.random.default_rng(7000 + 100 * case.p + case.n + case.C)
    mask = random_mask(rng, case.p)
    hyper = 10.0 ** rng.uniform(-2.0, 2.0, (case.C, 2 * case.p + 2))
    return mask, float(10.0 ** rng.uniform(-1.0, 0.5)), hyper
