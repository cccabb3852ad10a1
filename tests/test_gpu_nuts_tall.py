"""NUTS on the stepwise engine (logreg_amd/csrc/lr_tall_nuts.h; `mode="stepwise"`) on the MI355X: tall rows and wide models (p > 32), which
the fused kernel refuses.  The float64 kernel against the independent reference (tests/nuts_reference.py) transition by transition at
every padded width 4 .. 128, the float32 kernel against the float64 reference beyond the measured margin, rows that are genuinely off
chip, bytes (rerun, chunks, shards with mixed neighbours, the second build, the
streaming statistics), non-finite starts, the posterior and the planner.  The mode is accepted where the fused kernel has no variant (p > 32, or
rows beyond the LDS) and refused elsewhere, as before; so every narrow shape here has rows beyond the LDS.  Cases: tests/nuts_tall_cases.py."""
import collections
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import nuts_reference as nr
import nuts_tall_cases as tc

pytestmark = pytest.mark.gpu

SD = np.array([1.73, 0.065, 0.0068, 0.018, 0.023, 0.043, 0.55, 0.022])  # posterior scales of Pima: dmm = 1 / SD^2 is a unit-scale metric
FIELDS = ("n_leapfrog", "depth_sum", "accept_stat_sum", "divergent", "max_depth_hits")


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


EPS = 0.1  # under dmm = 1 / SD^2: acceptance statistic about 0.76, trees of depth about 5 (0.2 diverges: the correlations of Pima)


def kern(la, model, eps=EPS, max_depth=8):
    return la.nutsKernel(model.lpost, model.glp, eps=eps, dmm=1 / SD ** 2, max_depth=max_depth)


def run(la, k, q0, iters, thin=1, seed=7, mode="stepwise", **kw):
    cs = la.ChainSet(k, q0, seed=seed, mode=mode, **kw)
    d = la.DeviceArray(k.model.device, (iters, cs.C), np.int8)
    out = cs.advance(iters, thin, depth=d).to_host()
    return out, d.to_host(), cs


def against_reference(la, cases, dtype, margin):
    n = skipped = 0
    worst, mism, over = 0.0, [], []
    cnt, deep = collections.Counter(), collections.Counter()
    for case in cases:
        steps, refs = tc.kernel_vs_reference(la, case, dtype)
        assert steps[0]["x_out"].dtype == np.dtype(dtype)
        cn, cs, cm, cw = nr.compare(steps, refs, margin)
        n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
        if dtype == "float64":  # the bound of the case: nr.F64_TOL, but for the three tail cases named in tc.F64_SLICE_DEV
            print(f"  p={case.case.p} n={case.case.n} seed={case.case.seed}: {cw:.3g} (bound {tc.f64_tol(case):.3g})")
            over += [f"{case}: {cw:.3g} > {tc.f64_tol(case):.3g}"] if not cw <= tc.f64_tol(case) else []
        mism += [f"{case}: {m}" for m in cm]
        for row in refs:
            for r in row:
                cnt[r.reason] += 1
                deep[tc.padded(case.case.p)] += abs(r.depth) >= 7
    return n, skipped, worst, mism + over, cnt, deep


@pytest.mark.parametrize("widths", ["narrow", "wide"])
def test_float64_kernel_equals_the_reference_transition_by_transition(la, widths):
    """Teacher-forced: signed depth, leaf count and flags equal, state and acceptance statistic within nr.F64_TOL in every case -- all wide
    ones among them -- but three narrow cases of large steps from the tails, which exceeded it (9.09e-11, 1.27e-11, 1.18e-11) and whose
    bound is 10 x the deviation of the reference under slice-ordered sums from itself in that case (9.8e-10, 6.8e-11, 2.8e-10:
    tests/nuts_tall_cases.py f64_tol; measured on the CPU, as nr.F64_TOL was made).  A
    transition is left out only below a reference margin of nr.MIN_MARGIN, at most 1 in 1000 (the reference alone stays within that:
    tests/test_nuts_tall_cpu.py).  Every padded width reaches depth 7 and beyond; divergences, subtree and whole-tree U-turns occur."""
    cases = [c for c in tc.F64_CASES if (c.case.p > 32) == (widths == "wide")]
    n, skipped, worst, mism, cnt, deep = against_reference(la, cases, "float64", nr.MIN_MARGIN)
    print(f"{widths}: {n} transitions, {skipped} skipped, largest relative deviation {worst:.3g};", dict(cnt), "depth >= 7 per padded width:", dict(deep))
    assert not mism, "\n".join(mism[:20])
    assert skipped <= n / 1000
    assert widths == "narrow" or worst <= nr.F64_TOL
    assert all(deep[P] >= 3 for P in ((64, 128) if widths == "wide" else (4, 8, 16, 32))), dict(deep)
    for reason in (nr.DIVERGENCE, nr.SUBTREE, nr.TREE):
        assert cnt[reason] >= 5, dict(cnt)


@pytest.mark.parametrize("widths", ["narrow", "wide"])
def test_float32_kernel_equals_the_float64_reference_beyond_the_margin(la, widths):
    """As the fused kernel's float32 test: beyond the margin the signed depth, leaf count and flags are equal and the state and acceptance
    statistic agree to the tolerance.  p <= 32: nr.F32_TAU and nr.F32_STATE_TOL.  p > 32: the larger of those and 8 x what the
    reference's float32 mode showed against its float64 mode on the wide cases (tests/nuts_tall_cases.py; the old pair is the larger)."""
    cases, tau, tol = (tc.F32_WIDE, tc.F32_WIDE_TAU, tc.F32_WIDE_STATE_TOL) if widths == "wide" else (tc.F32_NARROW, nr.F32_TAU, nr.F32_STATE_TOL)
    n, skipped, worst, mism, _, _ = against_reference(la, cases, "float32", tau)
    print(f"float32 {widths}: {n} transitions, {skipped} below the margin {tau:g}, largest relative deviation {worst:.3g}")
    assert not mism, "\n".join(mism[:20])
    assert skipped <= 0.10 * n
    assert worst <= tol


def test_rows_that_are_off_chip(la):
    """n = 20 000 x p = 8: the automatic mode refuses it (rows beyond the LDS); the stepwise mode runs it in many row slices and agrees
    with the reference as above."""
    c = tc.OFF_CHIP.case
    X, y, ps, dmm, q0 = tc.problem(tc.OFF_CHIP)
    m = la.LogReg(X, y, ps, dtype="float64")
    k = la.nutsKernel(m.lpost, m.glp, eps=c.eps, dmm=dmm, max_depth=c.max_depth)
    with pytest.raises(la.LogregHipError, match="beyond"):
        la.mcmc(q0, k, iters=1, verb=False)
    plan = la.ChainSet(k, q0, seed=1, mode="stepwise").plan()
    assert plan["mode"] == "stepwise" and plan["group"] > 1 and plan["group"] * plan["rows_per_lane"] >= c.n
    n, skipped, worst, mism, _, _ = against_reference(la, [tc.OFF_CHIP], "float64", nr.MIN_MARGIN)
    print(f"off chip: plan {plan}, {n} transitions, {skipped} skipped, largest relative deviation {worst:.3g}")
    assert not mism, "\n".join(mism[:20])
    assert n == c.C * c.K and skipped <= n / 1000 and worst <= nr.F64_TOL


def _mixed_starts(rng, p, C):
    """ordinary, non-finite and tail starts, mixed among neighbours"""
    q0 = 0.3 * rng.standard_normal((C, p))
    kind = rng.integers(0, 3, C)
    q0[kind == 1, p // 2] = np.nan
    q0[kind == 2] *= 20.0
    return q0, kind


@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_bytes_rerun_chunks_shards_and_second_build(la, shape):
    """Rerun = run; chunks of 5 + 7 iterations = 12; a shard at chain_offset = lo with the slice count pinned to the whole run's equals
    the whole run's columns, with non-finite, tail and ordinary starts as neighbours; the second build gives equal bytes.  Both dtypes."""
    import altlib
    p, n, group, C = (8, 5001, 3, 300) if shape == "narrow" else (40, 100, 0, 150)  # (5001 rows: beyond the LDS in both dtypes)
    eps = 0.15 if shape == "wide" else 0.028
    X, y, ps = nr.synthetic_model(p, n, 100 + p)
    q0, kind = _mixed_starts(np.random.default_rng(5), p, C)
    for dtype in ("float32", "float64"):
        m = la.LogReg(X, y, ps, dtype=dtype)
        k = la.nutsKernel(m.lpost, m.glp, eps=eps, dmm=1.0, max_depth=5)
        full, dfull, cs = run(la, k, q0, 12, thin=2, group=group)
        cfull = cs.get_counters()
        pinned = cs.plan()["group"]
        assert cs.plan()["mode"] == "stepwise" and (group == 0 or pinned == group)
        assert np.all(dfull[:, kind == 1] == -1) and np.all(np.abs(dfull[:, kind != 1]) >= 1)
        again, dagain, _ = run(la, k, q0, 12, thin=2, group=group)
        assert full.tobytes() == again.tobytes() and dfull.tobytes() == dagain.tobytes()
        cs = la.ChainSet(k, q0, seed=7, mode="stepwise", group=group)
        parts = [cs.advance(it, 2).to_host() for it in (5, 7)]  # chunked: iter_offset
        assert np.concatenate(parts).tobytes() == full.tobytes()
        for f in ("n_leapfrog", "depth_sum", "divergent", "max_depth_hits"):
            assert np.array_equal(cs.get_counters()[f], cfull[f]), (dtype, f)
        np.testing.assert_allclose(cs.get_counters()["accept_stat_sum"], cfull["accept_stat_sum"], rtol=1e-13)  # (two partial sums added, not one sum)
        for lo, hi in ((1, 78), (131, 150)):
            sh, dsh, css = run(la, k, q0[lo:hi], 12, thin=2, chain_offset=lo, plan_chains=C, plan_first=0, group=pinned)
            assert sh.tobytes() == full[:, lo:hi].tobytes() and dsh.tobytes() == dfull[:, lo:hi].tobytes(), (dtype, lo, hi)
            for f in FIELDS:
                assert np.asarray(css.get_counters()[f]).tobytes() == np.ascontiguousarray(cfull[f][lo:hi]).tobytes(), (dtype, lo, hi, f)
        altlib.install()  # the second build of the same sources
        try:
            m_alt = la.LogReg(X, y, ps, dtype=dtype)
            alt, dalt, _ = run(la, la.nutsKernel(m_alt.lpost, m_alt.glp, eps=eps, dmm=1.0, max_depth=5), q0, 12, thin=2, group=group)
        finally:
            altlib.uninstall()
        assert full.tobytes() == alt.tobytes() and dfull.tobytes() == dalt.tobytes()


def test_statistics_and_summary_equal_those_of_the_kept_draws(la):
    X, y, ps = nr.synthetic_model(40, 100, 140)
    m = la.LogReg(X, y, ps, dtype="float64")
    k = la.nutsKernel(m.lpost, m.glp, eps=0.15, dmm=1.0, max_depth=5)
    q0 = 0.3 * np.random.default_rng(8).standard_normal((64, 40))
    cs = la.ChainSet(k, q0, seed=3, mode="stepwise")
    cs.enable_stats(5, 4)
    kept = np.concatenate([cs.advance(it, 2).to_host() for it in (8, 12)])
    summ = cs.stats_summary()
    np.testing.assert_allclose(summ["mean"], kept.mean(axis=(0, 1)), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(summ["sd"], kept.std(axis=(0, 1), ddof=1), rtol=1e-6)
    draws, info = la.mcmc(q0, k, thin=2, iters=20, verb=False, seed=3, mode="stepwise", return_info=True)
    assert draws.tobytes() == kept.tobytes() and info["plan"]["mode"] == "stepwise"
    only = la.mcmc(q0, k, thin=2, iters=20, verb=False, seed=3, mode="stepwise", summary_only=True)
    np.testing.assert_allclose(only["mean"], kept.mean(axis=(0, 1)), rtol=1e-9, atol=1e-12)
    assert np.array_equal(only["n_leapfrog"], info["n_leapfrog"]) and np.array_equal(only["divergent"], info["divergent"])
    assert np.array_equal(only["state"], info["state"])
    # an accumulator of kept draws sees the same draws and leaves the run as it is
    ac = la.Autocorr(64, 40, "float64")
    draws2, info2 = la.mcmc(q0, k, thin=2, iters=20, verb=False, seed=3, mode="stepwise", chunk=7, return_info=True, autocorr=ac)
    one = la.Autocorr(64, 40, "float64").update(kept)
    assert draws2.tobytes() == kept.tobytes() and ac.n_draws == 20 and "autocorr" in info2
    assert ac.sums()[0].tobytes() == one.sums()[0].tobytes() and ac.sums()[1].tobytes() == one.sums()[1].tobytes()
    ac.free(), one.free()


def test_checkpoint_and_resume_continue_the_same_chain(la):
    X, y, ps = nr.synthetic_model(17, 1501, 117)
    m = la.LogReg(X, y, ps, dtype="float32")
    k = la.nutsKernel(m.lpost, m.glp, eps=0.05, dmm=1.0, max_depth=5)
    q0 = 0.3 * np.random.default_rng(9).standard_normal((70, 17))
    cs = la.ChainSet(k, q0, seed=4, mode="stepwise", group=2)
    cs.advance(4, 2, keep=False)
    ck = cs.checkpoint()
    rest = cs.advance(6, 2).to_host()
    cs2 = la.ChainSet.resume(k, ck, group=2, mode="stepwise")
    assert cs2.plan() == cs.plan() and cs2.plan()["mode"] == "stepwise"
    assert cs2.advance(6, 2).to_host().tobytes() == rest.tobytes()
    for f in ("n_leapfrog", "depth_sum", "divergent", "max_depth_hits"):
        assert np.array_equal(cs2.get_counters()[f], cs.get_counters()[f]), f


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_start_finishes_in_place(la, bad):
    """a NaN or inf start does not move, is counted divergent, and does not stall its neighbours; the call returns within the step bound"""
    X, y, ps = nr.synthetic_model(65, 100, 165)
    m = la.LogReg(X, y, ps, dtype="float64")
    q0 = 0.2 * np.random.default_rng(2).standard_normal((64, 65))
    q0[::2, 3] = bad
    iters = 5
    out, dep, cs = run(la, la.nutsKernel(m.lpost, m.glp, eps=0.1, dmm=1.0, max_depth=10), q0, iters)
    cn, st = cs.get_counters(), cs.get_state()
    assert np.array_equal(st[::2], q0[::2], equal_nan=True)
    assert np.all(cn["divergent"][::2] == iters) and np.all(dep[:, ::2] == -1) and np.all(cn["n_leapfrog"][::2] == iters)
    assert np.all(np.isfinite(st[1::2])) and np.all(cn["divergent"][1::2] == 0) and np.all(np.abs(dep[:, 1::2]) >= 2)
    assert np.all(cn["n_leapfrog"] <= iters * (2 ** 10 - 1))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_posterior_matches_the_cpu_oracle(la, dtype):
    """A tall model (n = 5001 x p = 8, beyond the LDS in both dtypes), 1024 chains, 50 iterations discarded, 100 kept: pooled means and
    standard deviations against tests/golden/nuts_tall_posterior.json, the posterior of the same model from the CPU oracle's float64 HMC
    (its own code: no kernel of the library), |z| < 4.2 as the fused kernel's posterior test; divergences below 1 %.  (That test's
    posterior_hmc.json is of the 200-row Pima data, a shape that runs fused and is refused here.)"""
    gold = load_golden("nuts_tall_posterior.json")
    ref, beta, sd = gold["pooled"], np.array(gold["map"]), np.array(gold["laplace_sd"])
    X, y, ps = tc.POSTERIOR_MODEL()
    m = la.LogReg(X, y, ps, dtype=dtype)
    n_chains = 1024
    q0 = beta + sd * np.random.default_rng(1).standard_normal((n_chains, 8))
    cs = la.ChainSet(la.nutsKernel(m.lpost, m.glp, eps=0.5, dmm=1 / sd ** 2, max_depth=8), q0, seed=2024, mode="stepwise")
    cs.advance(1, 50, keep=False)
    summ = la.summarise(cs.advance(100, 1).to_host(), max_chains=128)
    info = cs.nuts_info()
    zm = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    se_sd = summ["sd"] / np.sqrt(2 * summ["ess"])
    zs = (summ["sd"] - np.array(ref["sd"])) / np.sqrt(se_sd ** 2 + np.array(ref["se_sd"]) ** 2)
    print(dtype, "z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2), "depth", info["mean_depth"].mean(), "accept stat", info["mean_accept_stat"].mean(),
          "divergent", info["divergent"].sum())
    assert cs.plan()["mode"] == "stepwise"
    assert np.max(np.abs(zm)) < 4.2 and np.max(np.abs(zs)) < 4.2
    assert info["divergent"].sum() < 0.01 * n_chains * 150 and info["mean_depth"].mean() > 2


def test_planner_on_the_device(la, models):
    from logreg_amd import _lib
    m = models["float32"]
    mode, group, rows = C.c_int32(), C.c_int32(), C.c_int32()
    rng = np.random.default_rng(0)
    tall = la.LogReg(rng.standard_normal((20000, 8)), (rng.random(20000) < 0.5).astype(float), 1.0)
    opts = _lib.RunOpts(n_chains=4096, mode=_lib.MODE_STEPWISE)
    _lib.check(tall._L.lr_plan_run(tall.handle, 4, C.byref(opts), C.byref(mode), C.byref(group), C.byref(rows)))
    assert _lib.MODE_NAMES[mode.value] == "stepwise" and group.value * rows.value >= 20000
    opts = _lib.RunOpts(n_chains=4096, mode=_lib.MODE_AUTO)  # unchanged: rows in LDS on 16 lanes per chain
    _lib.check(m._L.lr_plan_run(m.handle, 4, C.byref(opts), C.byref(mode), C.byref(group), C.byref(rows)))
    assert (mode.value, group.value) == (_lib.MODE_LDS, 16)
    # unchanged as well: a shape the fused kernel takes (Pima) refuses the stepwise mode
    with pytest.raises(la.LogregHipError, match="rows in LDS"):
        la.mcmc(np.zeros(8), kern(la, m), iters=1, verb=False, mode="stepwise")
    wide = la.LogReg(rng.standard_normal((100, 40)), (rng.random(100) < 0.5).astype(float), 1.0)
    kw = la.nutsKernel(wide.lpost, wide.glp, eps=0.1)
    with pytest.raises(la.LogregHipError, match="p = 40 > 32.*LR_MODE_STEPWISE"):
        la.mcmc(np.zeros(40), kw, iters=1, verb=False)
    assert la.ChainSet(kw, np.zeros(40), seed=1, mode="stepwise").plan()["mode"] == "stepwise"
    assert la.mcmc(np.zeros(40), kw, iters=2, thin=1, verb=False, mode="stepwise").shape == (2, 40)
    dense = la.nutsKernel(tall.lpost, tall.glp, eps=0.1, inv_metric=np.eye(8))
    with pytest.raises(la.LogregHipError, match="stepwise .tall-data. engine has no NUTS kernel"):
        la.mcmc(np.zeros(8), dense, iters=1, verb=False, mode="stepwise")
