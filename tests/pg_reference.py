"""A plain NumPy reference of the Polya-Gamma Gibbs sampler -- TEST INFRASTRUCTURE ONLY (a helper module, imported by the PG tests).

Written from the text of include/logreg_hip_pg.h and from nothing else.  It shares no arithmetic with the kernel
(logreg_amd/csrc/lr_pg.h) or the CPU test double (tests/host/lr_cpu_twin_pg.c):

* Philox4x32-10 is restated here on NumPy uint64 arrays, and a word is fetched by its index in the row's sequence (no cursor object);
* the draw runs on whole arrays under masks, with NumPy's / SciPy's exp, log, erfc and cos;
* A is one einsum over the rows, the factorisation is numpy.linalg.cholesky of the UNSCALED matrix, the mean comes from two triangular
  solves and the noise from a third (the kernel factorises the unit-diagonal scaling and sums entry by entry with fused multiply-adds).

`draw` also reports each draw's decision margin: the smallest relative gap |a - b| / max(|a|, |b|) of any comparison the draw made
(the choice of the left method z < 1 / t, U < r, the pair test, the two acceptance tests, X <= t, every squeeze comparison).
`dtype=np.float32` is the float32 mode: rows, psi, the arithmetic inside the draw and the stored state are NumPy float32; A, its
factorisation and the solves stay float64, as in the kernel.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.special import erfc

TAG = 0x10000000  # LR_PG_TAG
T_TRUNC = 0.64
MAX_ROUNDS, MAX_TRIALS, MAX_TERMS = 10, 160, 8

# ---- tolerances fixed on the CPU (tests/test_pg_cpu.py re-measures them; profiles/r21_pg.txt records the runs they come from)
# 10 x the largest relative deviation of omega and of the state between the test double and this reference over CPU_CASES
F64_TOL = 1.5e-13
# the float32 pair: 8 x the largest float64 margin at which this reference's float32 mode decided otherwise than its float64 mode, and
# 8 x the largest relative deviation of omega (of the state) where every decision agreed
F32_TAU = 1.1e-6
F32_OMEGA_TOL = 6.0e-5
F32_STATE_TOL = 7.5e-6

_M32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (uint64 holding 32-bit values) -> four arrays of words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _u(w, dt):
    return ((w >> np.uint64(8)).astype(np.float64) + 0.5).astype(dt) * dt(2.0 ** -24)


def normals(seed, chain, it, p):
    """the p standard normals of (seed, chain, iteration): normal blocks 0 .. ceil(p/4) - 1, Box-Muller pairs (w0, w1), (w2, w3); [C, p]"""
    chain = np.atleast_1d(np.asarray(chain, dtype=np.uint64))
    nb = (p + 3) // 4
    blk = np.arange(nb, dtype=np.uint64)[None, :]
    w = philox(chain[:, None], int(it) & 0xFFFFFFFF, (int(it) >> 32) & 0xFFFFFFFF, blk, seed, int(seed) >> 32)
    z = np.empty((chain.size, nb, 4))
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(_u(w[2 * h], np.float64)))
        th = 2.0 * np.pi * _u(w[2 * h + 1], np.float64)
        z[:, :, 2 * h], z[:, :, 2 * h + 1] = r * np.cos(th), r * np.sin(th)
    return z.reshape(chain.size, nb * 4)[:, :p]


def _gap(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isfinite(g), g, 0.0)


def _coef(n, x, small, dt):
    h = n + 0.5
    with np.errstate(all="ignore"):
        v = dt(2.0) / (dt(np.pi) * x)
        lo = dt(np.pi * h) * (v * np.sqrt(v)) * np.exp(dt(-2.0 * h * h) / x)
        hi = dt(np.pi * h) * np.exp(dt(-(h * h) * np.pi * np.pi * 0.5) * x)
    return np.where(small, lo, hi).astype(dt)


def draw(psi, seed, chain, it, row, dtype=np.float64):
    """omega ~ PG(1, |psi|) for arrays psi / chain / row (broadcast together) at iteration `it`: include/logreg_hip_pg.h "The draw".
    -> dict(omega, margin, proposals, terms), each of the broadcast shape; psi must be finite"""
    dt = np.dtype(dtype).type
    psi, chain, row = np.broadcast_arrays(np.asarray(psi, dtype=dt), np.asarray(chain, dtype=np.uint64), np.asarray(row, dtype=np.uint64))
    shape = psi.shape
    psi, chain, row = psi.ravel(), chain.ravel(), row.ravel()
    M = psi.size
    t = dt(T_TRUNC)
    it_lo, it_hi = int(it) & 0xFFFFFFFF, (int(it) >> 32) & 0xFFFFFFFF
    cursor = np.zeros(M, dtype=np.uint64)

    def word(idx):  # the next word of the sequences idx
        k = cursor[idx]
        blk = np.uint64(TAG) | ((k >> np.uint64(2)) << np.uint64(16)) | row[idx]
        w = philox(chain[idx], it_lo, it_hi, blk, seed, int(seed) >> 32)
        sel = (k & np.uint64(3)).astype(np.int64)
        cursor[idx] = k + np.uint64(1)
        return _u(np.choose(sel, w), dt)

    z = dt(0.5) * np.abs(psi)
    K = dt(np.pi * np.pi * 0.125) + dt(0.5) * z * z
    with np.errstate(all="ignore"):
        zc = np.minimum(z, dt(10.0))
        kt = (dt(np.pi * np.pi * 0.125) + dt(0.5) * zc * zc) * t
        pb = dt(0.5) * erfc(-((t * zc - dt(1.0)) / dt(0.8)) * dt(np.sqrt(0.5)))
        pa = dt(0.5) * erfc(((t * zc + dt(1.0)) / dt(0.8)) * dt(np.sqrt(0.5)))
        r = dt(1.0) / (dt(1.0) + dt(4.0 / np.pi) * (kt / t) * (np.exp(kt - zc) * pb + np.exp(kt + zc) * pa))
        r = np.where(z < dt(10.0), r, dt(0.0)).astype(dt)
        mu = dt(1.0) / z
    pair = z < dt(1.0) / t
    margin = _gap(z, dt(1.0) / t)
    X = np.full(M, t, dtype=dt)
    active = np.ones(M, dtype=bool)
    nprop, nterm = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)

    def note(idx, a, b):
        margin[idx] = np.minimum(margin[idx], _gap(a, b))

    for _ in range(MAX_ROUNDS):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        nprop[idx] += 1
        U = word(idx)
        right = U < r[idx]
        note(idx, U, r[idx])
        ir = idx[right]
        if ir.size:
            X[ir] = t + (-np.log(word(ir))) / K[ir]
        pend = idx[~right]
        for trial in range(MAX_TRIALS):
            if pend.size == 0:
                break
            ua, ub, uc = word(pend), word(pend), word(pend)
            ok = np.zeros(pend.size, dtype=bool)
            pm = pair[pend]
            ip = pend[pm]
            if ip.size:
                E1, E2 = -np.log(ua[pm]), -np.log(ub[pm])
                d = dt(1.0) + t * E1
                Xp = t / (d * d)
                lhs, rhs = E1 * E1, dt(2.0) * E2 / t
                alpha = np.exp(dt(-0.5) * z[ip] * z[ip] * Xp)
                first = lhs <= rhs
                note(ip, lhs, rhs)
                note(ip[first], uc[pm][first], alpha[first])
                X[ip] = Xp
                ok[pm] = first & (uc[pm] <= alpha)
            im = pend[~pm]
            if im.size:
                N = np.sqrt(dt(-2.0) * np.log(ua[~pm])) * np.cos(dt(2.0 * np.pi) * ub[~pm])
                w = dt(0.5) * mu[im] * (N * N)
                s = dt(1.0) + w + np.sqrt(w * (w + dt(2.0)))
                Xm = mu[im] / s
                thr = mu[im] / (mu[im] + Xm)
                note(im, uc[~pm], thr)
                Xm = np.where(uc[~pm] > thr, mu[im] * s, Xm).astype(dt)
                note(im, Xm, t)
                X[im] = Xm
                ok[~pm] = Xm <= t
            if trial == MAX_TRIALS - 1:
                X[pend] = np.minimum(X[pend], t)
            pend = pend[~ok]
        small = X[idx] <= t
        V = word(idx)
        S = _coef(0, X[idx], small, dt)
        Y = V * S
        und = np.arange(idx.size)
        rejected = np.zeros(idx.size, dtype=bool)
        for n in range(1, MAX_TERMS + 1):
            if und.size == 0:
                break
            nterm[idx[und]] += 1
            an = _coef(n, X[idx[und]], small[und], dt)
            with np.errstate(invalid="ignore"):
                if n & 1:
                    S[und] = S[und] - an
                    dec = Y[und] <= S[und]
                else:
                    S[und] = S[und] + an
                    dec = Y[und] > S[und]
                    rejected[und[dec]] = True
            note(idx[und], Y[und], S[und])
            und = und[~dec]
        active[idx[~rejected]] = False
    return {"omega": (dt(0.25) * X).reshape(shape), "margin": margin.reshape(shape), "proposals": nprop.reshape(shape), "terms": nterm.reshape(shape)}


@dataclass
class Sweep:
    beta: np.ndarray       # [C, p] the new states (the model's dtype)
    omega: np.ndarray      # [C, n]; NaN in the rows of a chain whose psi is not finite
    margin: np.ndarray     # [C, n] decision margins of the draws
    proposals: np.ndarray  # [C] what lr_pg_counters gains
    terms: np.ndarray
    skipped: np.ndarray    # [C] bool


def signed_rows(X, y, dtype=np.float64):
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    return ((2.0 * np.asarray(y, dtype=np.float64) - 1.0)[:, None] * X.astype(np.float64)).astype(dtype)


def sweep(Xs, pscale, beta, seed, chains, it, dtype=np.float64) -> Sweep:
    """one iteration of every chain: Xs [n, p] signed rows, beta [C, p], chains [C] global chain ids"""
    dt = np.dtype(dtype).type
    Xs = np.ascontiguousarray(Xs, dtype=dt)
    beta = np.atleast_2d(np.asarray(beta, dtype=dt))
    C, p = beta.shape
    n = Xs.shape[0]
    chains = np.asarray(chains, dtype=np.uint64)
    with np.errstate(all="ignore"):
        psi = (beta @ Xs.T).astype(dt)
    fin = np.isfinite(psi)
    d = draw(np.where(fin, psi, dt(0)), seed, chains[:, None], it, np.arange(n, dtype=np.uint64)[None, :], dtype)
    skipped = ~fin.all(axis=1)
    omega = np.where(fin, d["omega"], dt(np.nan)).astype(dt)
    X64 = Xs.astype(np.float64)
    b = 0.5 * X64.sum(axis=0)
    prior = np.diag(1.0 / np.broadcast_to(np.asarray(pscale, dtype=np.float64), (p,)) ** 2)
    z = normals(seed, chains, it, p)
    new = beta.astype(np.float64).copy()
    for c in range(C):
        if skipped[c]:
            continue
        A = np.einsum("n,nj,nk->jk", d["omega"][c].astype(np.float64), X64, X64) + prior
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            skipped[c] = True
            continue
        m = np.linalg.solve(L.T, np.linalg.solve(L, b))
        new[c] = m + np.linalg.solve(L.T, z[c])
    live = ~skipped
    return Sweep(new.astype(dt), omega, d["margin"], np.where(live, d["proposals"].sum(axis=1), 0), np.where(live, d["terms"].sum(axis=1), 0), skipped)


def run(Xs, pscale, beta, seed, chain_offset, iter_offset, iters, thin=1, dtype=np.float64):
    """`iters x thin` sweeps of every chain -> (kept [iters, C, p], proposals [C], terms [C], skipped [C])"""
    beta = np.atleast_2d(np.asarray(beta, dtype=dtype))
    C = beta.shape[0]
    chains = np.arange(C, dtype=np.uint64) + np.uint64(chain_offset)
    kept, prop, term, skip = [], np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    for i in range(iters * thin):
        s = sweep(Xs, pscale, beta, seed, chains, iter_offset + i, dtype)
        beta = s.beta
        prop, term, skip = prop + s.proposals, term + s.terms, skip + s.skipped
        if (i + 1) % thin == 0:
            kept.append(beta.copy())
    return np.array(kept), prop, term, skip


# ---- the shape set of the tests
@dataclass(frozen=True)
class Case:
    p: int
    n: int
    C: int
    seed: int = 20
    chain_offset: int = 5
    iter_offset: int = 11


# every width, every row count and every chain count of the issue at least once (the CPU set adds n = 1 and n = 257)
CPU_CASES = (Case(3, 1, 3), Case(4, 15, 65), Case(5, 17, 257), Case(8, 200, 65), Case(9, 257, 3), Case(16, 15, 257), Case(17, 17, 1), Case(31, 200, 3),
             Case(32, 257, 1), Case(32, 17, 65))
GPU_CASES = (Case(3, 15, 257), Case(4, 17, 65), Case(5, 200, 3), Case(8, 200, 65), Case(9, 15, 1), Case(16, 17, 257), Case(17, 200, 3), Case(31, 15, 65),
             Case(32, 17, 257), Case(32, 200, 1))
F32_CASES = tuple(Case(c.p, min(c.n, 40) if c.n != 200 else 40, c.C) for c in GPU_CASES)  # n <= 40: whole chains must clear the margin


def make_case(case: Case):
    """-> (X [n, p], y [n], pscale [p], states [C, p]): a design with an intercept, labels from a random coefficient vector, and states
    spread so that |psi| / 2 falls on both sides of 1 / t and of 10"""
    rng = np.random.default_rng(1000 * case.p + 10 * case.n + case.C)
    X = rng.standard_normal((case.n, case.p))
    X[:, 0] = 1.0
    truth = rng.standard_normal(case.p) / np.sqrt(case.p)
    y = (rng.random(case.n) < 1.0 / (1.0 + np.exp(-X @ truth))).astype(np.float64)
    pscale = rng.uniform(0.5, 5.0, case.p)
    spread = rng.choice([0.3, 3.0, 12.0], size=(case.C, 1))
    states = truth + spread * rng.standard_normal((case.C, case.p)) / np.sqrt(case.p)
    return X, y, pscale, states


def rel_dev(a, b):
    """largest |a - b| relative to the larger magnitude of the pair's row (a chain's state, a chain's omega): [..., k] -> scalar"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.max(np.abs(b), axis=-1, keepdims=True), 1e-300)
    return float(np.max(np.abs(a - b) / scale)) if a.size else 0.0


def omega_dev(a, b):
    """largest elementwise relative deviation of two omega arrays"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0
