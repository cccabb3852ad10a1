"""Two plain references of one NUTS transition under a DENSE metric -- TEST INFRASTRUCTURE ONLY (a helper module, imported by the dense
NUTS tests).  Written from the definition in include/logreg_hip_dense.h and from nothing else; neither shares arithmetic with the kernel
(logreg_amd/csrc/lr_nuts_dense.h), with the library's factorisation (csrc/lr_dense.h: the factors here come from numpy.linalg.cholesky)
or with `kernels._numpy_nuts`, and they share nothing with each other beyond the random stream:

(a) `transition_whitened`: the existing `nuts_reference.transition` with the UNIT metric on the whitened problem.  With C = diag(s) L
    (Sigma = C C^T):  theta' = C^-1 theta,  lpost'(theta') = lpost(C theta'),  glp'(theta') = C^T glp(C theta'),  the same normals z.
    Dense NUTS with inverse metric Sigma and p = C^-T z IS this transition mapped back by theta = C theta': no matrix ever touches a
    momentum, a kinetic energy or a U-turn product.

(b) `transition_dense`: the transition in plain space with the products of the definition -- p = (A z) / s, v = s o (R (s o p)),
    H = -lpost + p . v / 2, the generalised criterion on Sigma rho' -- momenta kept in lists, every sum `math.fsum` (float64 mode) as
    `nuts_reference` does for the diagonal metric.  `dtype=np.float32` is its float32 mode: states, momenta, the factors s, 1 / s, R, A,
    the products and dot products in NumPy float32, energies and draws in float64 as in the kernel.

The tolerances of the GPU tests (tests/test_gpu_nuts_dense.py) are what (a) against (b) shows on the CPU (tests/test_nuts_dense_cpu.py
re-measures them; profiles/r19_nuts_dense.txt records the run): none comes from the kernel.
"""
from __future__ import annotations

import collections
import math

import numpy as np

import nuts_reference as nr
from nuts_reference import DIVERGENCE, MAX_DEPTH, MERGE2, MERGE3, MERGE23, SUBTREE, TREE, Transition, _colsum, _fsum, _lae

MIN_MARGIN = nr.MIN_MARGIN  # float64: a transition may be left out only below this reference margin (at most 1 in 1000)
# Measured on the CPU by measure_f64() / measure_f32() below (`python tests/nuts_dense_reference.py`; profiles/r19_nuts_dense.txt);
# tests/test_nuts_dense_cpu.py re-measures and fails if a constant is smaller than what it finds.
DENSE_F64_TOL = 1.212e-11  # 10 x the largest relative deviation between (a) and (b) (1.2113e-12, rounded up, over the 6480 transitions of DENSE_CASES x METRICS)
DENSE_F32_TAU = 1.567e-6   # 8 x the largest float64 margin at which (b)'s float32 mode disagreed with its float64 mode (1.958e-07: 1 disagreement
                           # in 861 120 transitions of F32_CASES x METRICS at 130 chains under 184 seeds)
DENSE_F32_STATE_TOL = 5.775e-4  # ... and 8 x their largest relative deviation where they agreed (7.219e-05, same runs)

METRICS = ("dense", "diag", "unit")


def factors(sigma):
    """-> s, R, L, A = L^-T, C = diag(s) L of a symmetric positive definite Sigma, by NumPy (float64)"""
    sigma = np.asarray(sigma, dtype=np.float64)
    s = np.sqrt(np.diag(sigma))
    R = sigma / np.outer(s, s)
    R = 0.5 * (R + R.T)
    np.fill_diagonal(R, 1.0)
    L = np.linalg.cholesky(R)
    A = np.linalg.inv(L).T
    return s, R, L, A, s[:, None] * L


def transition_whitened(lpost, glp, x, eps, sigma, max_depth, stream) -> Transition:
    """(a): nuts_reference.transition, unit metric, on the whitened problem; the state mapped back"""
    _, _, _, _, Cm = factors(sigma)
    xw = np.linalg.solve(Cm, np.asarray(x, dtype=np.float64))
    t = nr.transition(lambda w: lpost(Cm @ w), lambda w: Cm.T @ np.asarray(glp(Cm @ w), dtype=np.float64), xw, eps, 1.0, max_depth, stream)
    moved = t.prop_leaf >= 0
    t.x = Cm @ t.x if moved else np.asarray(x, dtype=np.float64).copy()
    return t


def transition_dense(lpost, glp, x, eps, sigma, max_depth, stream, dtype=np.float64) -> Transition:
    """(b): one NUTS iteration in plain space under the inverse metric Sigma (include/logreg_hip_dense.h "Definition")"""
    dt = np.float64 if np.dtype(dtype) == np.float64 else np.float32
    f64 = dt is np.float64
    x = np.asarray(x, dtype=dt)
    s64, R64, _, A64, _ = factors(sigma)
    s, si, R, A = s64.astype(dt), (1.0 / s64).astype(dt), R64.astype(dt), A64.astype(dt)
    step, heps = dt(float(eps)), dt(0.5 * float(eps))

    def product(M, u):
        if f64:
            return np.array([_fsum((M[i] * u).tolist()) for i in range(len(u))])
        return (M @ u).astype(dt)

    def dot(a, b):
        t = (a * b).astype(dt)
        return _fsum(t.tolist()) if f64 else float(np.sum(t, dtype=dt))

    def velocity(p):
        return (s * product(R, (s * p).astype(dt))).astype(dt)

    def kinetic(p):
        return dot(p, velocity(p))

    margin = [math.inf]

    def note(m):
        if m < margin[0]:
            margin[0] = m

    def turning(a, b, rho):
        w = velocity((rho - dt(0.5) * (a + b)).astype(dt))
        sa, sb = dot(a, w), dot(b, w)
        nw = float(np.linalg.norm(w.astype(np.float64)))
        m = math.inf
        for sv, v in ((sa, a), (sb, b)):
            den = float(np.linalg.norm(v.astype(np.float64))) * nw
            m = min(m, abs(sv) / den if den > 0 and math.isfinite(den) else 0.0)
        note(m)
        return sa <= 0 or sb <= 0

    with np.errstate(all="ignore"):
        lp = float(lpost(x))
        g = np.asarray(glp(x), dtype=dt)
        z = np.asarray(stream.normals(), dtype=np.float64).astype(dt)
        p0 = (product(A, z) * si).astype(dt)
        H0 = _fsum((0.5 * kinetic(p0), -lp))
        tree_p = [p0]
        ends = {-1: (x, p0, g), 1: (x, p0, g)}
        W, prop, prop_k = 0.0, x, -1
        acc, n_leaf, depth = [], 0, 0
        for d in range(max_depth):
            depth = d + 1
            sgn = stream.direction(d)
            q, p, g = ends[sgn]
            p_inner_old, p_outer_old = p, ends[-sgn][1]
            sub_p, sub_prop, sub_k, Ws = [], None, -1, 0.0
            for i in range(2 ** d):
                k = n_leaf
                p = (p + dt(sgn) * heps * g).astype(dt)
                q = (q + dt(sgn) * step * velocity(p)).astype(dt)
                lpl, g = float(lpost(q)), np.asarray(glp(q), dtype=dt)
                p = (p + dt(sgn) * heps * g).astype(dt)
                n_leaf += 1
                delta = _fsum((0.5 * kinetic(p), -lpl, -H0))
                if not math.isfinite(delta) or delta > 1000.0:
                    if math.isfinite(delta):
                        note(abs(delta - 1000.0) / 1000.0)
                    acc.append(0.0)
                    return Transition(prop, -depth, n_leaf, math.fsum(acc) / n_leaf, True, False, DIVERGENCE, margin[0], 0, prop_k)
                note(abs(delta - 1000.0) / 1000.0)
                acc.append(1.0 if delta <= 0.0 else math.exp(-delta))
                sub_p.append(p)
                if i == 0:
                    Ws, sub_prop, sub_k = -delta, q, k
                else:
                    Wn = _lae(Ws, -delta)
                    u, prob = stream.leaf_u(k), math.exp(-delta - Wn)
                    note(abs(u - prob))
                    if u < prob:
                        sub_prop, sub_k = q, k
                    Ws = Wn
                spans, length = [], 2
                while (i + 1) % length == 0:
                    first = i + 1 - length
                    if turning(sub_p[first], sub_p[i], _colsum(sub_p[first:i + 1], dt)):
                        spans.append(length)
                    length *= 2
                if spans:
                    return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, False, SUBTREE, margin[0], min(spans), prop_k)
            u, prob = stream.merge_u(d), math.exp(min(Ws - W, 700.0))
            note(abs(u - prob))
            if u < prob:
                prop, prop_k = sub_prop, sub_k
            W = _lae(W, Ws)
            rho_old, rho_sub = _colsum(tree_p, dt), _colsum(sub_p, dt)
            tree_p = tree_p + sub_p if sgn > 0 else sub_p[::-1] + tree_p
            ends[sgn] = (q, p, g)
            rho = _colsum(tree_p, dt)
            p_first, p_outer_new = sub_p[0], sub_p[-1]
            t1 = turning(ends[-1][1], ends[1][1], rho)
            t2 = turning(p_outer_old, p_first, (rho_old + p_first).astype(dt))
            t3 = turning(p_outer_new, p_inner_old, (rho_sub + p_inner_old).astype(dt))
            if t1 or t2 or t3:
                reason = TREE if t1 else (MERGE23 if t2 and t3 else (MERGE2 if t2 else MERGE3))
                return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, False, reason, margin[0], 0, prop_k)
        return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, True, MAX_DEPTH, margin[0], 0, prop_k)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "p n eps max_depth C K seed chain_offset iter_offset start_scale")


def _cases():
    """The shape set of nuts_reference.GPU_F64_CASES -- every width class of the kernel on both sides of its boundary, 1 / 3 / 65 / 257
    chains (partial waves, more than one workgroup), a few dozen rows, max_depth 10, non-zero chain and iteration offsets (the high
    iteration word among them) -- with chain and iteration counts cut to what a test of seconds can restate: per width a small-step
    case (deep trees: the second leaf-uniform block at leaf 64, checkpoints up to index 8) and a large-step case from the tails
    (divergences and early stops beside building chains)."""
    deep = {3: (65, 1, 0.02), 4: (3, 6, 0.03), 5: (3, 6, 0.01), 8: (65, 1, 0.01), 9: (3, 6, 0.02), 16: (65, 1, 0.03), 17: (3, 6, 0.02),
            31: (1, 10, 0.02), 32: (65, 1, 0.03)}
    cases = []
    for i, (p, (C, K, eps)) in enumerate(deep.items()):
        n = (21, 37, 45, 53)[i % 4]
        cases.append(Case(p, n, eps, 10, C, K, 300 + i, 11 * i + 1, 2 ** 32 * (i % 2) + i + 1, 1.0))
        cases.append(Case(p, n, (1.6, 0.6, 2.2)[i % 3], 10, (257, 3, 65, 1)[i % 4], 2, 400 + i, 5 + i, 1 + i, 3.0))
    return cases


DENSE_CASES = _cases()
# float32: the widths and row counts of nuts_reference.F32_CASES; starts within the bulk (0.3: from further out the acceptance statistic
# of a first iteration falls to 1e-70, where its RELATIVE deviation measures nothing) and a quarter of those steps (trees of 15 - 60
# leaves: every leaf adds decisions that float32 rounding can move)
F32_CASES = [Case(p, n, 0.25 * eps, 10, 65, 2, 500 + i, 7 * i + 1, 3 + i, 0.3)
             for i, (p, n, eps) in enumerate(((3, 203, 0.15), (8, 157, 0.12), (9, 301, 0.1), (16, 119, 0.1), (17, 251, 0.08), (32, 185, 0.08)))]


def random_correlation(p, rng, cond=100.0):
    """a random correlation matrix of condition number <= cond: random orthogonal directions, eigenvalues log-uniform in a range whose
    ratio is sqrt(cond), rescaled to the unit diagonal (the rescaling can widen the ratio; sqrt leaves room, and the bound is checked)"""
    if p == 1:
        return np.ones((1, 1))
    Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    lam = np.exp(rng.uniform(0.0, 0.5 * math.log(cond), p))
    M = (Q * lam) @ Q.T
    d = np.sqrt(np.diag(M))
    R = M / np.outer(d, d)
    R = 0.5 * (R + R.T)
    np.fill_diagonal(R, 1.0)
    assert np.linalg.cond(R) <= cond
    return R


def case_sigma(case, metric):
    """the inverse metric of (case, metric): "dense" = D R D (random correlation of condition number <= 100, D in [0.3, 3]),
    "diag" = D^2 alone, "unit" = I"""
    rng = np.random.default_rng(7000 + 10 * case.p + case.seed)
    R = random_correlation(case.p, rng)
    D = rng.uniform(0.3, 3.0, case.p)
    if metric == "dense":
        return R * np.outer(D, D)
    if metric == "diag":
        return np.diag(D * D)
    assert metric == "unit"
    return np.eye(case.p)


def case_problem(case, float32=False):
    """-> X, y, pscale, q0 [C, p] (float32=True: X and q0 rounded to float32, as float64 values)"""
    X, y, ps = nr.synthetic_model(case.p, case.n, 100 + case.p)
    q0 = case.start_scale * np.random.default_rng(1000 * case.p + case.max_depth + case.seed).standard_normal((case.C, case.p))
    if float32:
        return X.astype(np.float32).astype(np.float64), y, ps, q0.astype(np.float32).astype(np.float64)
    return X, y, ps, q0


def stream_of(case, k, c):
    return nr.PhiloxStream(case.seed, case.chain_offset + c, case.iter_offset + k, case.p)


def run_stepwise_dense(la, model, q0, K, eps, sigma, max_depth, seed, chain_offset=0, iter_offset=0, **chainset_kw):
    """nuts_reference.run_stepwise for the dense kernel: K iterations at thin 1 through the Python face, one launch per iteration"""
    k = la.nutsKernel(model.lpost, model.glp, eps=eps, max_depth=max_depth, inv_metric=sigma)
    x = np.ascontiguousarray(np.atleast_2d(q0), dtype=model.np_dtype)
    steps = []
    for it in range(K):
        cs = la.ChainSet(k, x, seed=seed, chain_offset=chain_offset, **chainset_kw)
        cs.iter_offset = iter_offset + it
        d = la.DeviceArray(model.device, (1, cs.C), np.int8)
        out = cs.advance(1, 1, depth=d).to_host()[0]
        cn = cs.get_counters()
        steps.append(dict(x_in=x, x_out=out, depth=d.to_host()[0].astype(int), **{f: np.array(cn[f]) for f in
                          ("n_leapfrog", "divergent", "max_depth_hits", "accept_stat_sum")}))
        x = out
    return steps


def reference_steps_whitened(lpost, glp, steps, case, sigma):
    """(a) for every (k, chain) of `steps`, each from the implementation's own input state"""
    return [[transition_whitened(lpost, glp, np.asarray(s["x_in"][c], dtype=np.float64), case.eps, sigma, case.max_depth, stream_of(case, k, c))
             for c in range(s["x_in"].shape[0])] for k, s in enumerate(steps)]


def as_steps(rows):
    """reference transitions [k][c] in the shape nuts_reference.compare takes for an implementation's steps"""
    return [dict(x_in=np.array([t.x_in for t in row]), x_out=np.array([t.x for t in row]), depth=np.array([t.depth for t in row]),
                 n_leapfrog=np.array([t.n_leaf for t in row]), divergent=np.array([int(t.divergent) for t in row]),
                 max_depth_hits=np.array([int(t.hit) for t in row]), accept_stat_sum=np.array([t.accept_stat for t in row])) for row in rows]


def measure_f64(cases=None, metrics=METRICS):
    """(a) against (b) in float64 along (a)'s chain.  -> dict: n, skipped (margin of (a) below MIN_MARGIN), mismatches, worst (largest
    relative deviation of state or acceptance statistic), reasons, deep (transitions of depth >= 7 per padded width)"""
    from oracle.oracle import OracleModel
    n = skipped = 0
    worst, mism = 0.0, []
    reasons, deep = collections.Counter(), collections.Counter()
    for case in cases or DENSE_CASES:
        X, y, ps, q0 = case_problem(case)
        om = OracleModel(X, y, ps)
        P = 4 if case.p <= 4 else 8 if case.p <= 8 else 16 if case.p <= 16 else 32
        for metric in metrics:
            sigma = case_sigma(case, metric)
            x, rows_a, rows_b = q0, [], []
            for k in range(case.K):
                ra, rb = [], []
                for c in range(case.C):
                    ta = transition_whitened(om.lpost, om.glp, x[c], case.eps, sigma, case.max_depth, stream_of(case, k, c))
                    tb = transition_dense(om.lpost, om.glp, x[c], case.eps, sigma, case.max_depth, stream_of(case, k, c))
                    ta.x_in = tb.x_in = x[c]
                    ta.margin = min(ta.margin, tb.margin)  # a decision near its threshold in either restatement
                    ra.append(ta)
                    rb.append(tb)
                    reasons[ta.reason] += 1
                    deep[P] += abs(ta.depth) >= 7
                rows_a.append(ra)
                rows_b.append(rb)
                x = np.array([t.x for t in ra])
            cn, cs, cm, cw = nr.compare(as_steps(rows_b), rows_a, MIN_MARGIN)
            n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
            mism += [f"{case} {metric}: {m}" for m in cm]
    return dict(n=n, skipped=skipped, mismatches=mism, worst=worst, reasons=reasons, deep=deep)


def measure_f32(cases=None, metrics=METRICS):
    """(b) in NumPy float32 against (b) in float64, teacher-forced along the float32 chain, as nuts_reference.measure_float32_mode.
    -> dict: n, disagree, tau (largest float64 margin among the disagreements), dev (largest relative deviation among the others),
    margins"""
    from oracle.oracle import OracleModel
    tau = dev = 0.0
    margins, disagree = [], 0
    for case in cases or F32_CASES:
        X, y, ps, q0 = case_problem(case, float32=True)
        m32, m64 = nr.F32Model(X, y, ps), OracleModel(X, y, ps)
        for metric in metrics:
            sigma = case_sigma(case, metric)
            x = q0.astype(np.float32)
            for k in range(case.K):
                nxt = []
                for c in range(case.C):
                    t32 = transition_dense(m32.lpost, m32.glp, x[c], case.eps, sigma, case.max_depth, stream_of(case, k, c), dtype=np.float32)
                    t64 = transition_dense(m64.lpost, m64.glp, x[c].astype(np.float64), case.eps, sigma, case.max_depth, stream_of(case, k, c))
                    nxt.append(t32.x)
                    margins.append(t64.margin)
                    if nr.shape_of(t32) != nr.shape_of(t64) or t32.prop_leaf != t64.prop_leaf:
                        disagree += 1
                        tau = max(tau, t64.margin)
                    else:
                        a, b = np.asarray(t32.x, dtype=np.float64), np.asarray(t64.x, dtype=np.float64)
                        dev = max(dev, float(np.max(np.abs(a - b)) / np.max(np.abs(b))),
                                  abs(t32.accept_stat - t64.accept_stat) / t64.accept_stat if t64.accept_stat > 0 else 0.0)
                x = np.array(nxt, dtype=np.float32)
    margins = np.array(margins)
    return dict(n=len(margins), disagree=disagree, tau=tau, dev=dev, margins=margins)


def _f32_one(args):
    case, rep = args
    return measure_f32([case._replace(C=130, seed=case.seed + 1000 * rep)])


if __name__ == "__main__":
    # python tests/nuts_dense_reference.py [replicates]: the measurements behind the constants above.  Float64: DENSE_CASES x METRICS as
    # the test runs them.  Float32: F32_CASES widened to 130 chains under `replicates` seeds (default 8), in 16 processes.
    import multiprocessing
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    m = measure_f64()
    print(f"float64 (a) vs (b): {m['n']} transitions, {m['skipped']} skipped below {MIN_MARGIN:g}, {len(m['mismatches'])} mismatches, largest relative "
          f"deviation {m['worst']:.4g} (x 10 = {10 * m['worst']:.4g}); reasons {dict(m['reasons'])}; depth >= 7 per width {dict(m['deep'])}")
    for line in m["mismatches"][:10]:
        print("   ", line)
    with multiprocessing.Pool(16) as pool:
        res = pool.map(_f32_one, [(c, r) for r in range(reps) for c in F32_CASES], chunksize=1)
    tau, dev = max(r["tau"] for r in res), max(r["dev"] for r in res)
    mg = np.concatenate([r["margins"] for r in res])
    print(f"float32 (b) vs float64 (b): {len(mg)} transitions, {sum(r['disagree'] for r in res)} disagree; largest disagreeing margin {tau:.4g} "
          f"(x 8 = {8 * tau:.4g}); largest relative deviation {dev:.4g} (x 8 = {8 * dev:.4g}); share of margins below 8 x tau {np.mean(mg < 8 * tau):.5f}")


# ---- the warm-up under a dense metric (include/logreg_hip_dense.h "Warm-up") -------------------------------------------------------------
def warm_dense(model, q0, W, *, sigma0=None, seed=5, chain_offset=0, cuts=None, on_device=False, adapt_metric=True, eps0=0.0, max_depth=5, L=None):
    """adapt_cases.warm for lr_dense_adapt_*: one warm-up of `model` from q0 [C, p], `cuts` = the iterations of each run call.
    -> dict(state, out [W,C,p], depth [W,C], astat [W,C], counters, eps, sigma [p,p], info, trace [W,5], metric [windows,p,p])"""
    import ctypes as C
    from logreg_amd import DeviceArray, _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_dense(_lib.bind_adapt(model._L if L is None else L))
    Cn, p = q0.shape
    dt = model.np_dtype
    st = np.array(q0, dtype=dt, order="C")
    s0 = None if sigma0 is None else np.ascontiguousarray(sigma0, dtype=np.float64)
    o = _lib.AdaptOpts(W=W, adapt_metric=int(adapt_metric), eps0=eps0, dmm0=None)
    h = C.c_void_p()
    _lib.check(L.lr_dense_adapt_create(model.handle, Cn, C.byref(o), None if s0 is None else s0.ctypes.data, C.byref(h)))
    try:
        host = {"state": st, "out": np.zeros((W, Cn, p), dtype=dt), "depth": np.zeros((W, Cn), dtype=np.int8), "astat": np.zeros((W, Cn), dtype=np.float64),
                "counters": np.zeros(Cn, dtype=NUTS_COUNTERS)}
        dev = {k: DeviceArray.from_host(model.device, v) for k, v in host.items()} if on_device else None
        opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, seed=seed, group=0, mode=_lib.MODE_AUTO, on_device=int(on_device))
        t = 0
        for k in (cuts or [W]):
            def ptr(name, per_iter):
                return (dev[name].ptr if on_device else host[name].ctypes.data) + t * per_iter
            _lib.check(L.lr_dense_adapt_run(h, ptr("state", 0), k, max_depth, C.byref(opts), ptr("out", Cn * p * st.itemsize), ptr("counters", 0), ptr("depth", Cn),
                                            ptr("astat", Cn * 8)))
            t += k
        e, info = C.c_double(), _lib.AdaptInfo()
        sigma = np.empty((p, p))
        _lib.check(L.lr_dense_adapt_result(h, C.byref(e), sigma.ctypes.data, C.byref(info)))
        trace = np.zeros((W, _lib.ADAPT_TRACE_COLS))
        metric = np.zeros((info.n_windows, p, p))
        _lib.check(L.lr_dense_adapt_trace(h, trace.ctypes.data, metric.ctypes.data if info.n_windows else None))
        if on_device:
            _lib.check(L.lr_stream_sync(model.device, None))
            host = {k: v.to_host() for k, v in dev.items()}
            for v in dev.values():
                v.free()
    finally:
        L.lr_dense_adapt_destroy(h)
    return {**host, "eps": e.value, "sigma": sigma, "trace": trace, "metric": metric,
            "info": {"iterations": info.iterations, "metric_skipped": info.metric_skipped, "windows": info.windows, "n_windows": info.n_windows}}


def same_bytes(a, b, keys=("state", "out", "depth", "astat", "trace", "metric", "sigma", "counters")):
    """the first key whose bytes differ between two results of warm_dense(), or None"""
    for k in keys:
        if a[k].tobytes() != b[k].tobytes():
            return k
    return None if np.float64(a["eps"]).tobytes() == np.float64(b["eps"]).tobytes() and a["info"] == b["info"] else "result"


def sigma_of_window(x):
    """One window: x [L, C, p] (any float dtype; converted exactly) -> dict(n, S, sigma, tol [p, p], finite): the regularised inverse
    metric of include/logreg_hip_dense.h in np.longdouble straight from the draws (two passes, no Chan merge), and the error bound of
    the device's float64 arithmetic derived from the inputs alone, as adapt_reference.metric_of bounds the variance (u = 2^-53):
        the co-moment M_jl is a sum of N products d_j d_l, each formed with a few roundings and added along paths no longer than N:
        (N + 4) u sum |d_j d_l| <= (N + 4) u sqrt(M_jj M_ll) (Cauchy-Schwarz); every mean the device subtracts carries an error of at
        most dm_j = (N + 4) u max|x_j|, and moving the means of a decomposition sum_b n_b (mean_b - mean)_j (mean_b - mean)_l + within
        by dm changes it by at most dm_j sqrt(N M_ll) + dm_l sqrt(N M_jj) + 2 N dm_j dm_l;
        S = M / (N - 1) and Sigma = a S + c I add one division, a product and a sum: 2 u |S| and 4 u |Sigma| on top.
    On the diagonal this is adapt_reference.metric_of's tol_var and tol_inv."""
    U = 2.0 ** -53
    xl = np.asarray(x).astype(np.longdouble).reshape(-1, np.shape(x)[-1])
    N, p = xl.shape
    with np.errstate(all="ignore"):
        mean = xl.sum(axis=0) / N
        d = xl - mean
        M = d.T @ d
        S = M / (N - 1)
        a, c = np.longdouble(N) / (N + 5), np.longdouble(1e-3) * 5 / (N + 5)
        sigma = a * S + c * np.eye(p)
        xmax = np.max(np.abs(np.where(np.isfinite(xl), xl, 0)), axis=0)
        dm = (N + 4) * U * xmax
        dg = np.diag(M)
        tol_M = (N + 4) * U * np.sqrt(np.outer(dg, dg)) + np.outer(dm, np.sqrt(N * dg)) + np.outer(np.sqrt(N * dg), dm) + 2 * N * np.outer(dm, dm)
        tol_S = tol_M / max(N - 1, 1) + 2 * U * np.abs(S)
        tol = a * tol_S + 4 * U * np.abs(sigma)
    s64 = sigma.astype(np.float64)
    return {"n": N, "S": S.astype(np.float64), "sigma": s64, "tol": tol.astype(np.float64) + U * np.abs(s64), "finite": bool(np.all(np.isfinite(s64)))}
