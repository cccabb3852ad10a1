"""NUTS under a dense metric (logreg_amd/csrc/lr_nuts_dense.h, include/logreg_hip_dense.h) on the MI355X.

1. The float64 kernel, teacher-forced, against reference (a) of tests/nuts_dense_reference.py (the unit-metric reference on the whitened
   problem) over dr.DENSE_CASES x (dense, diagonal, unit): decisions equal, states within dr.DENSE_F64_TOL; the float32 kernel against
   the float64 reference beyond the float32 margin.  None of the bounds comes from the kernel (tests/test_nuts_dense_cpu.py).
2. A diagonal Sigma and Sigma = I against lr_run_nuts with dmm = 1 / diag: the same decisions, states within dr.DENSE_F64_TOL.
3. Bytes: a rerun, chunks, shards at odd offsets, host against device pointers, the second build, fresh models.
4. Non-finite starts mixed into the waves.
5. Pima: the Laplace metric with a step-size warm-up against the golden posterior; the dense warm-up against the diagonal one.
6. The warm-up: every iteration replayed through lr_run_nuts_dense, every window's Sigma recomputed in NumPy within a bound derived
   from the inputs, the step sizes against adapt_reference's dual averaging, cut invariance, a window whose Sigma is refused."""
import collections
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import adapt_cases
import adapt_reference as ar
import nuts_dense_reference as dr
import nuts_reference as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    if logreg_amd.device_count() <= 0:
        pytest.skip("no GPU")
    return logreg_amd


@pytest.fixture(scope="module")
def models(la, pima, pscale):
    X, y = pima
    return {d: la.LogReg(X, y, pscale, dtype=d) for d in ("float32", "float64")}


@pytest.fixture(scope="module")
def pima_sigma(la, models, map_beta):
    return la.laplace_metric(models["float64"], map_beta)


def kern(la, model, sigma, eps=0.2, max_depth=8):
    return la.nutsKernel(model.lpost, model.glp, eps=eps, max_depth=max_depth, inv_metric=sigma)


def run(la, k, q0, iters, thin=1, seed=7, **kw):
    cs = la.ChainSet(k, q0, seed=seed, **kw)
    d = la.DeviceArray(k.model.device, (iters, cs.C), np.int8)
    out = cs.advance(iters, thin, depth=d).to_host()
    return out, d.to_host(), cs


@pytest.fixture(scope="module")
def kernel_vs_reference(la):
    """dr.DENSE_CASES x dr.METRICS on the float64 kernel and reference (a) from the kernel's own inputs"""
    from oracle.oracle import OracleModel
    res = []
    for case in dr.DENSE_CASES:
        X, y, ps, q0 = dr.case_problem(case)
        model = la.LogReg(X, y, ps, dtype="float64")
        om = OracleModel(X, y, ps)
        for metric in dr.METRICS:
            sigma = dr.case_sigma(case, metric)
            steps = dr.run_stepwise_dense(la, model, q0, case.K, case.eps, sigma, case.max_depth, case.seed, case.chain_offset, case.iter_offset)
            res.append((case, metric, sigma, model, steps, dr.reference_steps_whitened(om.lpost, om.glp, steps, case, sigma)))
    return res


def test_float64_kernel_equals_the_whitened_reference_at_every_width(kernel_vs_reference):
    """Signed depth, leaf count and flags equal, state and acceptance statistic within dr.DENSE_F64_TOL (10 x the deviation between the
    two CPU references).  A transition is left out only below a reference margin of 1e-9, at most 1 in 1000.  Depth >= 7 at least 10
    times per padded width; at least 20 each of divergence, subtree and tree stops."""
    n = skipped = 0
    worst, mism = 0.0, []
    cnt, deep = collections.Counter(), collections.Counter()
    for case, metric, _, _, steps, refs in kernel_vs_reference:
        cn, cs, cm, cw = nr.compare(steps, refs, dr.MIN_MARGIN)
        n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
        mism += [f"{case} {metric}: {m}" for m in cm]
        P = 4 if case.p <= 4 else 8 if case.p <= 8 else 16 if case.p <= 16 else 32
        for row in refs:
            for r in row:
                cnt[r.reason] += 1
                deep[P] += abs(r.depth) >= 7
    print(f"dense kernel vs reference (a): {n} transitions, {skipped} skipped, largest relative deviation {worst:.3g} (bound {dr.DENSE_F64_TOL:g});", dict(cnt),
          "depth >= 7 per padded width:", dict(deep))
    assert not mism, "\n".join(mism[:20])
    assert skipped <= n / 1000
    assert worst <= dr.DENSE_F64_TOL
    assert all(deep[P] >= 10 for P in (4, 8, 16, 32)), dict(deep)
    for reason in (nr.DIVERGENCE, nr.SUBTREE, nr.TREE):
        assert cnt[reason] >= 20, dict(cnt)
    assert {c.p for c, *_ in kernel_vs_reference} == {3, 4, 5, 8, 9, 16, 17, 31, 32}
    assert {c.C for c, *_ in kernel_vs_reference} == {1, 3, 65, 257}


def test_diagonal_and_unit_sigma_reduce_to_the_diagonal_sampler(la, kernel_vs_reference):
    """lr_run_nuts with dmm = 1 / diag(Sigma), teacher-forced from the dense kernel's inputs: depths and counters equal, states and
    acceptance statistics within dr.DENSE_F64_TOL (not bytes: p . (c p) and (p . p) c round differently)."""
    n, worst = 0, 0.0
    for case, metric, sigma, model, steps, _ in kernel_vs_reference:
        if metric == "dense":
            continue
        diag = nr.run_stepwise(la, model, steps[0]["x_in"], case.K, case.eps, 1.0 / np.diag(sigma), case.max_depth, case.seed, case.chain_offset, case.iter_offset,
                               forced=steps)
        for k, (g, t) in enumerate(zip(steps, diag)):
            for f in ("depth", "n_leapfrog", "divergent", "max_depth_hits"):
                assert np.array_equal(g[f], t[f]), (case, metric, k, f, np.argwhere(g[f] != t[f])[:10].tolist())
            a, b = g["x_out"].astype(np.float64), t["x_out"].astype(np.float64)
            dev = np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), 1e-300)
            sa, sb = g["accept_stat_sum"], t["accept_stat_sum"]
            dev = np.maximum(dev, np.where(sb > 0, np.abs(sa - sb) / np.where(sb > 0, sb, 1.0), 0.0))
            worst = max(worst, float(np.max(dev)))
            n += len(dev)
    print(f"diagonal / unit Sigma against lr_run_nuts: {n} transitions, largest relative deviation {worst:.3g} (bound {dr.DENSE_F64_TOL:g})")
    assert n > 1000 and worst <= dr.DENSE_F64_TOL


def test_float32_kernel_equals_the_float64_reference_beyond_the_margin(la):
    """The float32 kernel teacher-forced against reference (a) in float64 on the float32-rounded data and state.  Where the reference's
    margin exceeds dr.DENSE_F32_TAU the signed depth, leaf count and flags are equal and the state and acceptance statistic agree to
    dr.DENSE_F32_STATE_TOL: 8 x what reference (b)'s NumPy-float32 mode showed against its float64 mode on the CPU.  At most 10 % of the
    transitions fall below the margin."""
    from oracle.oracle import OracleModel
    n = skipped = 0
    worst, mism = 0.0, []
    for case in dr.F32_CASES:
        X, y, ps, q0 = dr.case_problem(case, float32=True)
        model = la.LogReg(X, y, ps, dtype="float32")
        om = OracleModel(X, y, ps)
        for metric in dr.METRICS:
            sigma = dr.case_sigma(case, metric)
            steps = dr.run_stepwise_dense(la, model, q0, case.K, case.eps, sigma, case.max_depth, case.seed, case.chain_offset, case.iter_offset)
            assert steps[0]["x_out"].dtype == np.float32
            refs = dr.reference_steps_whitened(om.lpost, om.glp, steps, case, sigma)
            cn, cs, cm, cw = nr.compare(steps, refs, dr.DENSE_F32_TAU)
            n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
            mism += [f"{case} {metric}: {m}" for m in cm]
    print(f"float32 dense kernel vs float64 reference: {n} transitions, {skipped} below the margin {dr.DENSE_F32_TAU:g}, largest relative deviation {worst:.3g} "
          f"(bound {dr.DENSE_F32_STATE_TOL:g})")
    assert not mism, "\n".join(mism[:20])
    assert skipped <= 0.10 * n
    assert worst <= dr.DENSE_F32_STATE_TOL


def test_bit_exact_rerun_chunks_shards_pointers_and_second_build(la, models, map_beta, pima, pscale, pima_sigma):
    """Samples, depths and counters as bytes: a rerun; chunked against monolithic; shards whose first chain is 1, 2, 3 (mod 4) with odd
    lengths under plan_chains; one iteration from host pointers against device pointers; the second build of the same sources."""
    import altlib
    rng = np.random.default_rng(5)
    Cn = 500
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((Cn, 8))
    fields = ("n_leapfrog", "depth_sum", "accept_stat_sum", "divergent", "max_depth_hits")
    for dtype in ("float32", "float64"):
        k = kern(la, models[dtype], pima_sigma)
        full, dfull, cs0 = run(la, k, q0, 12, thin=2)
        cfull = cs0.get_counters()
        assert np.all(np.abs(dfull) >= 1) and len(np.unique(np.abs(dfull))) > 1
        again, dagain, _ = run(la, k, q0, 12, thin=2)
        assert full.tobytes() == again.tobytes() and dfull.tobytes() == dagain.tobytes()
        cs = la.ChainSet(k, q0, seed=7)
        parts = [cs.advance(n, 2).to_host() for n in (5, 7)]  # chunked: iter_offset
        assert np.concatenate(parts).tobytes() == full.tobytes()
        for lo, hi in ((1, 78), (202, 333), (303, 500), (498, 499)):
            assert lo % 4 in (1, 2, 3) and (hi - lo) % 2 == 1
            sh, dsh, css = run(la, k, q0[lo:hi], 12, thin=2, chain_offset=lo, plan_chains=Cn, plan_first=0)
            assert sh.tobytes() == full[:, lo:hi].tobytes() and dsh.tobytes() == dfull[:, lo:hi].tobytes(), (dtype, lo, hi)
            csh = css.get_counters()
            for f in fields:
                assert np.asarray(csh[f]).tobytes() == np.ascontiguousarray(cfull[f][lo:hi]).tobytes(), (dtype, lo, hi, f)
        via_mcmc = la.mcmc(q0[202:333], k, thin=2, iters=12, verb=False, seed=7, chain_offset=202, plan_chains=Cn, plan_first=0)
        assert via_mcmc.tobytes() == full[:, 202:333].tobytes()
        # host pointers (the kernel called as a function: one iteration, staged) against device pointers (a ChainSet)
        one, _, _ = run(la, k, q0, 1, seed=11)
        k2 = kern(la, models[dtype], pima_sigma)
        k2._seed = 11
        assert k2(q0).astype(models[dtype].np_dtype).tobytes() == one[0].tobytes()
        altlib.install()  # the second build of the same sources
        try:
            m_alt = la.LogReg(*pima, pscale, dtype=dtype)
            alt, dalt, _ = run(la, kern(la, m_alt, pima_sigma), q0, 12, thin=2)
        finally:
            altlib.uninstall()
        assert full.tobytes() == alt.tobytes() and dfull.tobytes() == dalt.tobytes()


def test_fresh_models_chunked_equals_monolithic(la):
    rng = np.random.default_rng(11)
    for t in range(12):
        n, p = int(rng.integers(20, 300)), int(rng.integers(2, 33))
        X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
        y = (rng.random(n) < 0.5).astype(float)
        dtype = ("float32", "float64")[t % 2]
        m = la.LogReg(X, y, np.full(p, 2.0), dtype=dtype)
        sigma = dr.random_correlation(p, rng) * 0.25
        k = la.nutsKernel(m.lpost, m.glp, eps=0.1, max_depth=6, inv_metric=sigma)
        q0 = 0.1 * rng.standard_normal((96, p))
        full, dfull, _ = run(la, k, q0, 6, seed=t)
        cs = la.ChainSet(k, q0, seed=t)
        parts = np.concatenate([cs.advance(2, 1).to_host(), cs.advance(4, 1).to_host()])
        assert full.tobytes() == parts.tobytes(), (t, n, p, dtype)
        assert np.all(np.abs(dfull) >= 1)
        # the same chains under another metric on the same model and stream: the factor image is replaced, not reused
        k2 = la.nutsKernel(m.lpost, m.glp, eps=0.1, max_depth=6, inv_metric=np.eye(p) * 0.25)
        other, _, _ = run(la, k2, q0, 6, seed=t)
        assert other.tobytes() != full.tobytes()
        back, _, _ = run(la, k, q0, 6, seed=t)
        assert back.tobytes() == full.tobytes()
        m.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_start_finishes_in_place(la, models, map_beta, pima_sigma, bad):
    """non-finite and ordinary chains mixed inside every wave (a wave holds four chains): the former finish at depth -1 where they are"""
    q0 = np.tile(map_beta, (66, 1))
    stuck = np.arange(66) % 3 == 0
    q0[stuck, 3] = bad
    iters = 5
    out, dep, cs = run(la, kern(la, models["float64"], pima_sigma), q0, iters)
    cn, st = cs.get_counters(), cs.get_state()
    assert np.array_equal(st[stuck], q0[stuck], equal_nan=True)
    assert np.all(cn["divergent"][stuck] == iters) and np.all(dep[:, stuck] == -1)
    assert np.all(np.isfinite(st[~stuck])) and np.all(cn["divergent"][~stuck] == 0) and np.all(dep[:, ~stuck] >= 1)
    clean, dclean, _ = run(la, kern(la, models["float64"], pima_sigma), np.tile(map_beta, (66, 1)), iters)
    assert out[:, ~stuck].tobytes() == clean[:, ~stuck].tobytes() and dep[:, ~stuck].tobytes() == dclean[:, ~stuck].tobytes()  # untouched by their neighbours


def z_scores(summ, ref):
    zm = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    se_sd = summ["sd"] / np.sqrt(2 * summ["ess"])
    zs = (summ["sd"] - np.array(ref["sd"])) / np.sqrt(se_sd ** 2 + np.array(ref["se_sd"]) ** 2)
    return zm, zs


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_pima_laplace_metric_and_dense_against_diagonal_warmup(la, models, map_beta, pima_sigma, dtype):
    """256 chains.  (1) optimize.laplace_metric, a step-size-only warm-up under it, 200 sampling iterations: posterior mean and sd
    against tests/golden/posterior_hmc.json by the z-score rule of test_gpu_nuts.py::test_posterior_matches_the_reference.
    (2) nuts_warmup_dense against nuts_warmup from eps = 1 and the unit metric, same seed and W = 300: the dense run's mean leapfrog
    count per sampling iteration must be strictly lower (no ratio fixed in advance; the figures are in profiles/r19_nuts_dense.txt)."""
    ref = load_golden("posterior_hmc.json")["pooled"]
    model = models[dtype]
    rng = np.random.default_rng(41)
    q0 = map_beta + 0.5 * np.array(ref["sd"]) * rng.standard_normal((256, 8))
    lap = la.nuts_warmup_dense(model.lpost, model.glp, q0, 100, inv_metric=pima_sigma, adapt_metric=False, seed=43)
    assert np.array_equal(lap.inv_metric, pima_sigma) and lap.info["windows"] == 0 and lap.trace[0, 0] == 1.0 and lap.kernel.params["eps"] == lap.eps
    out, info = la.mcmc(lap.state, lap.kernel, thin=1, iters=200, verb=False, seed=47, return_info=True)
    zm, zs = z_scores(la.summarise(out, max_chains=128), ref)
    steps_lap = float(info["n_leapfrog"].mean()) / 200
    print(f"PIMA {dtype} laplace metric: eps {lap.eps:.4g} depth {float(np.mean(info['mean_depth'])):.3f} leapfrogs / iteration {steps_lap:.2f} "
          f"accept {float(np.mean(info['mean_accept_stat'])):.3f} divergent {int(info['divergent'].sum())} z(mean) {np.round(zm, 2)} z(sd) {np.round(zs, 2)}")
    assert np.max(np.abs(zm)) < 4.2 and np.max(np.abs(zs)) < 4.2
    assert info["divergent"].sum() < 0.01 * 256 * 200
    W = 300
    dense = la.nuts_warmup_dense(model.lpost, model.glp, q0, W, seed=43)
    diag = la.nuts_warmup(model.lpost, model.glp, q0, W, seed=43)
    assert dense.trace[0, 0] == 1.0 == diag.trace[0, 0] and dense.info["windows"] == 3 == diag.info["windows"] and dense.info["metric_skipped"] == 0
    got = {}
    for name, res in (("dense", dense), ("diag", diag)):
        o2, i2 = la.mcmc(res.state, res.kernel, thin=1, iters=200, verb=False, seed=47, return_info=True)
        got[name] = float(i2["n_leapfrog"].mean()) / 200
        z2, _ = z_scores(la.summarise(o2, max_chains=128), ref)
        print(f"PIMA {dtype} {name} warm-up: eps {res.eps:.4g} depth {float(np.mean(i2['mean_depth'])):.3f} leapfrogs / iteration {got[name]:.2f} "
              f"accept {float(np.mean(i2['mean_accept_stat'])):.3f} divergent {int(i2['divergent'].sum())} max |z(mean)| {np.max(np.abs(z2)):.2f}")
        assert np.max(np.abs(z2)) < 4.2
    assert got["dense"] < got["diag"], got
    # the adapted matrix is the posterior's: its correlations against the Laplace approximation's (a sanity condition, 0.2 absolute)
    cor = lambda s: s / np.sqrt(np.outer(np.diag(s), np.diag(s)))  # noqa: E731
    assert np.max(np.abs(cor(dense.inv_metric) - cor(pima_sigma))) < 0.2


# ---- the warm-up ---------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(la, p, dtype):
    if (p, dtype) not in _MODELS:
        X, y, ps = adapt_cases.data(p)
        _MODELS[(p, dtype)] = la.LogReg(X, y, ps, dtype=dtype)
    return _MODELS[(p, dtype)]


def sigma_at(res, W, sigma0):
    """[W, p, p]: the inverse metric iteration t ran with, from the metric rows of the trace"""
    _, ends = ar.schedule(W)
    out = np.tile(np.asarray(sigma0, dtype=np.float64), (W, 1, 1))
    for k, e in enumerate(ends[:len(res["metric"])]):
        out[e:] = res["metric"][k]
    return out


def plain_iteration(model, state, eps, sigma, t, seed, chain_offset=0, max_depth=adapt_cases.MAX_DEPTH):
    """one lr_run_nuts_dense iteration at the warm-up's Philox index -> (state, depth [C], counters [C])"""
    from logreg_amd import _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_dense(model._L)
    st = np.array(state, dtype=model.np_dtype, order="C")
    Cn = st.shape[0]
    depth = np.zeros((1, Cn), dtype=np.int8)
    cnt = np.zeros(Cn, dtype=NUTS_COUNTERS)
    s = np.ascontiguousarray(sigma, dtype=np.float64)
    opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, iter_offset=_lib.ADAPT_ITER_BASE + t, seed=seed, group=0, mode=_lib.MODE_AUTO, on_device=0)
    _lib.check(L.lr_run_nuts_dense(model.handle, st.ctypes.data, float(eps), max_depth, s.ctypes.data, C.byref(opts), None, cnt.ctypes.data, depth.ctypes.data))
    return st, depth[0], cnt


def replay(model, q0, res, W, seed, sigma0, chain_offset=0):
    sig = sigma_at(res, W, sigma0)
    moved = 0
    for t in range(W):
        prev = np.array(q0 if t == 0 else res["out"][t - 1], dtype=model.np_dtype)
        st, depth, cnt = plain_iteration(model, prev, res["trace"][t, 0], sig[t], t, seed, chain_offset)
        assert st.tobytes() == res["out"][t].tobytes(), t
        assert np.array_equal(depth, res["depth"][t]), t
        assert cnt["accept_stat_sum"].tobytes() == res["astat"][t].tobytes(), t
        moved += bool(np.any(res["astat"][t] > 0))
    return moved


@pytest.mark.parametrize("dtype,Cn,p", [("float32", 1, 8), ("float32", 3, 20), ("float64", 5, 16), ("float64", 3, 3)])
def test_every_warmup_iteration_is_the_plain_dense_kernel(la, dtype, Cn, p):
    """W = 150 (one window, 75 .. 100): every iteration replayed by a one-iteration lr_run_nuts_dense at the trace's (eps_t, Sigma_t),
    compared as bytes -- the TUNED instantiation is the plain one, and the factor the handle uploads at the window's end is the one
    lr_run_nuts_dense makes of the traced Sigma."""
    W = 150
    model = model_of(la, p, dtype)
    q0 = adapt_cases.start(Cn, p)
    sigma0 = dr.random_correlation(p, np.random.default_rng(p)) * 0.5
    res = dr.warm_dense(model, q0, W, sigma0=sigma0, seed=5)
    assert res["state"].tobytes() == res["out"][-1].tobytes()
    if Cn * 25 > p + 1:  # enough draws for a matrix that differs from the start
        assert res["info"]["windows"] == 1 and not np.array_equal(res["sigma"], sigma0)
    assert np.array_equal(res["sigma"], res["metric"][-1])
    assert replay(model, q0, res, W, 5, sigma0) > W // 2


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("Cn,p,W", [(1, 3, 150), (65, 8, 150), (257, 16, 60), (1025, 20, 260), (3, 8, 19)])
def test_teacher_forced_dense_adaptation(la, dtype, Cn, p, W):
    """From the device's own acceptance statistics and states: abar_t and the step sizes against adapt_reference's dual averaging at
    adapt_cases.EPS_RTOL (the tolerance of tests/test_gpu_adapt.py), and every window's Sigma recomputed in np.longdouble from the kept
    draws within dr.sigma_of_window's bound, which is derived from the inputs alone."""
    model = model_of(la, p, dtype)
    res = dr.warm_dense(model, adapt_cases.start(Cn, p), W, seed=17)
    tf = ar.teacher_forced(res["astat"], res["out"], W, np.ones(p))
    tr = res["trace"]
    assert np.all(np.abs(tr[:, 1] - tf["abar"]) <= tf["tol_abar"])
    assert np.array_equal(tr[:, 3], tf["window"]) and np.array_equal(tr[:, 4], tf["n"])
    dev = max(np.max(np.abs(tr[:, 0] - tf["eps"]) / tf["eps"]), np.max(np.abs(tr[:, 2] - tf["log_eps_bar"]) / np.maximum(np.abs(tf["log_eps_bar"]), 1.0)),
              abs(res["eps"] - tf["final"]) / tf["final"])
    init, ends = ar.schedule(W)
    assert res["info"] == {"iterations": W, "metric_skipped": 0, "windows": len(ends), "n_windows": len(ends)}
    start, worst = init, 0.0
    for k, e in enumerate(ends):
        want = dr.sigma_of_window(res["out"][start:e])
        assert want["finite"] and want["n"] == Cn * (e - start)
        err = np.abs(res["metric"][k] - want["sigma"])
        worst = max(worst, float(np.max(err / want["tol"])))
        assert np.all(err <= want["tol"]), (k, float(np.max(err / want["tol"])))
        assert np.all(want["tol"] <= 1e-9 * np.sqrt(np.outer(np.diag(want["sigma"]), np.diag(want["sigma"]))))  # tight enough to tell a wrong kernel
        assert np.array_equal(res["metric"][k], res["metric"][k].T)
        start = e
    print(f"DENSE WARMUP {dtype} C{Cn}_p{p}_W{W}: step-size deviation {dev:.3e}, Sigma error {worst:.3g} of its bound, moving {int(np.sum(tr[:, 1] > 0))} of {W}")
    assert dev <= adapt_cases.EPS_RTOL, dev
    assert tr[0, 0] == 1.0 and np.sum(tr[:, 1] > 0) > W // 2


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_warmup_cut_invariance_determinism_and_a_refused_window(la, dtype):
    import altlib
    Cn, p, W = 65, 8, 150
    model = model_of(la, p, dtype)
    q0 = adapt_cases.start(Cn, p)
    one = dr.warm_dense(model, q0, W, seed=23)
    assert one["info"]["windows"] == 1 and one["info"]["metric_skipped"] == 0
    for name, kw in (("1 + 7 + 142", dict(cuts=[1, 7, 142])), ("a cut at the window's end", dict(cuts=[100, 50])), ("150 single calls", dict(cuts=[1] * W)),
                     ("device pointers", dict(on_device=True)), ("device pointers in pieces", dict(on_device=True, cuts=[1, 98, 2, 49])), ("twice over", dict())):
        assert dr.same_bytes(one, dr.warm_dense(model, q0, W, seed=23, **kw)) is None, name
    assert dr.same_bytes(one, dr.warm_dense(model, q0, W, seed=24)) is not None
    altlib.install()  # the second build of the same sources
    try:
        X, y, ps = adapt_cases.data(p)
        m_alt = la.LogReg(X, y, ps, dtype=dtype)
        alt = dr.warm_dense(m_alt, q0, W, seed=23)
        m_alt.close()
    finally:
        altlib.uninstall()
    assert dr.same_bytes(one, alt) is None
    # step size only: Sigma_0 stays, no window
    sigma0 = dr.random_correlation(p, np.random.default_rng(3)) * 0.5
    fixed = dr.warm_dense(model, q0, W, sigma0=sigma0, seed=23, adapt_metric=False)
    assert fixed["sigma"].tobytes() == sigma0.tobytes() and fixed["info"]["n_windows"] == 0 == fixed["info"]["windows"] and np.all(fixed["trace"][:, 3] == -1)
    tf = ar.teacher_forced(fixed["astat"], fixed["out"], W, np.ones(p), adapt_metric=False)
    assert np.max(np.abs(fixed["trace"][:, 0] - tf["eps"]) / tf["eps"]) <= adapt_cases.EPS_RTOL and abs(fixed["eps"] - tf["final"]) <= adapt_cases.EPS_RTOL * tf["final"]
    # A window whose Sigma is refused keeps the previous metric.  The regularised Sigma = a S + c I of finite draws is positive definite
    # whatever S is (S is positive semi-definite, c > 0) -- equal starts or a tiny W cannot make it fail; what can is a state that is not
    # finite: one chain starts at NaN (finite input data; the chain stays where it is), its coordinate's co-moments are NaN.
    bad = q0.copy()
    bad[5, 1] = np.nan
    W2 = 60
    res = dr.warm_dense(model, bad, W2, sigma0=sigma0, seed=29)
    assert res["info"] == {"iterations": W2, "metric_skipped": 1, "windows": 1, "n_windows": 1}
    assert res["sigma"].tobytes() == sigma0.tobytes() and res["metric"][0].tobytes() == sigma0.tobytes()
    assert np.all(res["astat"][:, 5] == 0.0) and np.all(np.isnan(res["out"][:, 5, 1])) and np.all(np.isfinite(np.delete(res["out"], 5, axis=1)))
