"""The fused NUTS kernel (logreg_amd/csrc/lr_nuts.h, include/logreg_hip_nuts.h) on the MI355X: step parity with the CPU test double of
the same ABI, the posterior against the reference's, bit exactness of reruns / chunks / shards / the second build, the saturated
BlackJAX setting, non-finite starts, fresh models and the planner.

Against the independent reference (tests/nuts_reference.py: one transition restated without the checkpoint scheme): the float64 kernel
transition by transition at p = 3 .. 32 (every width class, 1 / 3 / 65 / 257 chains, trees to depth 7 and beyond) and, at the same
inputs, against the double; the float32 kernel against the float64 reference wherever the reference's decision margin exceeds the
measured float32 threshold; shards that start at chain ids 1, 2, 3 (mod 4) with odd lengths and mixed neighbours (non-finite, tail
and ordinary starts) against the whole run, bytes for bytes."""
import collections
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import nuts_reference as nr

pytestmark = pytest.mark.gpu

PRE = np.array([10.0, 1, 1, 1, 1, 1, 5, 1])  # fit-blackjax-nuts.py:101 `pre`; dmm = 1 / pre
EPS = 0.002  # the stable step below which the posterior test runs (about 0.003 diverges on Pima with this metric)


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


def kern(la, model, eps=EPS, max_depth=10):
    return la.nutsKernel(model.lpost, model.glp, eps=eps, dmm=1 / PRE, max_depth=max_depth)


def run(la, k, q0, iters, thin=1, seed=7, depth=True, **kw):
    cs = la.ChainSet(k, q0, seed=seed, **kw)
    d = la.DeviceArray(k.model.device, (iters, cs.C), np.int8) if depth else None
    out = cs.advance(iters, thin, depth=d).to_host()
    return out, (d.to_host() if depth else None), cs


def z_scores(summ, ref):
    zm = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    se_sd = summ["sd"] / np.sqrt(2 * summ["ess"])
    zs = (summ["sd"] - np.array(ref["sd"])) / np.sqrt(se_sd ** 2 + np.array(ref["se_sd"]) ** 2)
    return zm, zs


def test_step_parity_with_the_test_double(la, models, pima, pscale, map_beta):
    """float64, 256 chains x 20 iterations at thin 1 through the same ABI: every depth, divergence flag and counter equal.  The states
    agree to 1e-7 relative: about 5000 leapfrog steps per chain carry the different summation orders of the two sums (measured:
    3e-8 at most, in 30 of 40 960 values; 1e-9 holds for all but those)."""
    import twin_nuts
    rng = np.random.default_rng(3)
    sd = np.array([1.73, 0.065, 0.0068, 0.018, 0.023, 0.043, 0.55, 0.022])
    q0 = map_beta + 0.5 * sd * rng.standard_normal((256, 8))
    out_g, dep_g, cs_g = run(la, kern(la, models["float64"]), q0, 20, precision="full")
    cnt_g = cs_g.get_counters()
    twin_nuts.install()
    try:
        X, y = pima
        mt = la.LogReg(X, y, pscale, dtype="float64")
        out_t, dep_t, cs_t = run(la, kern(la, mt), q0, 20)
        cnt_t = cs_t.get_counters()
    finally:
        twin_nuts.uninstall()
    assert np.array_equal(dep_g, dep_t), np.argwhere(dep_g != dep_t)[:10]
    assert np.array_equal(cnt_g["n_leapfrog"], cnt_t["n_leapfrog"]) and np.array_equal(cnt_g["divergent"], cnt_t["divergent"])
    assert np.array_equal(cnt_g["max_depth_hits"], cnt_t["max_depth_hits"])
    np.testing.assert_allclose(out_g, out_t, rtol=1e-7, atol=1e-12)
    assert np.mean(np.abs(out_g - out_t) <= 1e-9 * np.abs(out_t)) > 0.99
    np.testing.assert_allclose(cnt_g["accept_stat_sum"], cnt_t["accept_stat_sum"], rtol=1e-7)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_posterior_matches_the_reference(la, models, map_beta, dtype):
    ref = load_golden("posterior_hmc.json")["pooled"]
    C = 4096
    cs = la.ChainSet(kern(la, models[dtype]), np.tile(map_beta, (C, 1)), seed=2024)
    cs.advance(1, 100, keep=False)  # away from the common start
    samples = cs.advance(100, 1).to_host()
    info = cs.nuts_info()
    summ = la.summarise(samples, max_chains=128)
    zm, zs = z_scores(summ, ref)
    print(dtype, "z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2), "depth", info["mean_depth"].mean(), "accept stat",
          info["mean_accept_stat"].mean(), "divergent", info["divergent"].sum())
    assert np.max(np.abs(zm)) < 4.2 and np.max(np.abs(zs)) < 4.2
    assert info["divergent"].sum() < 0.01 * C * 200


def test_bit_exact_rerun_chunks_shards_and_second_build(la, models, map_beta, pima, pscale):
    import altlib
    rng = np.random.default_rng(5)
    C = 1000
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((C, 8))
    for dtype in ("float32", "float64"):
        k = kern(la, models[dtype], max_depth=8)
        full, dfull, _ = run(la, k, q0, 12, thin=2)
        again, dagain, _ = run(la, k, q0, 12, thin=2)
        assert np.array_equal(full, again) and np.array_equal(dfull, dagain)
        cs = la.ChainSet(k, q0, seed=7)
        parts = [cs.advance(n, 2).to_host() for n in (5, 7)]  # chunked: iter_offset
        assert np.array_equal(np.concatenate(parts), full)
        lo, hi = 300, 650  # a shard of the same planned run
        sh = la.mcmc(q0[lo:hi], k, thin=2, iters=12, verb=False, seed=7, chain_offset=lo, plan_chains=C, plan_first=0)
        assert np.array_equal(sh, full[:, lo:hi])
        altlib.install()  # the second build of the same sources: bytes compared
        try:
            m_alt = la.LogReg(*pima, pscale, dtype=dtype)
            alt, dalt, _ = run(la, kern(la, m_alt, max_depth=8), q0, 12, thin=2)
        finally:
            altlib.uninstall()
        assert full.tobytes() == alt.tobytes() and dfull.tobytes() == dalt.tobytes()


def test_saturation_at_the_blackjax_setting(la, models, map_beta):
    """eps = 1e-3 with the BlackJAX `pre`: the counters against the loop's bound, iteration by iteration."""
    C, iters, md = 512, 6, 10
    out, dep, cs = run(la, kern(la, models["float32"], eps=1e-3, max_depth=md), np.tile(map_beta, (C, 1)), iters)
    cn = cs.get_counters()
    depth = np.abs(dep.astype(np.int64))
    assert depth.min() >= 1 and depth.max() <= md
    assert np.array_equal(cn["depth_sum"], depth.sum(axis=0))
    assert np.array_equal(cn["divergent"], (dep < 0).sum(axis=0))
    full = (2 ** depth - 1)  # a tree that stops at depth d took at most 2^d - 1 steps, and more than 2^(d-1) - 1
    assert np.all(cn["n_leapfrog"] <= full.sum(axis=0)) and np.all(cn["n_leapfrog"] >= (2 ** (depth - 1)).sum(axis=0))
    sat = cn["max_depth_hits"] == iters  # chains whose every tree reached max_depth without turning: exactly 1023 steps each
    assert np.all(cn["n_leapfrog"][sat] == iters * (2 ** md - 1))
    print("BlackJAX setting: mean depth", depth.mean(), "saturated chains", sat.mean(), "steps / iteration", cn["n_leapfrog"].mean() / iters)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_start_finishes_in_place(la, models, map_beta, bad):
    q0 = np.tile(map_beta, (64, 1))
    q0[::2, 3] = bad
    iters = 5
    out, dep, cs = run(la, kern(la, models["float64"]), q0, iters)
    cn = cs.get_counters()
    st = cs.get_state()
    assert np.array_equal(st[::2], q0[::2], equal_nan=True)
    assert np.all(cn["divergent"][::2] == iters) and np.all(dep[:, ::2] == -1)
    assert np.all(np.isfinite(st[1::2])) and np.all(cn["divergent"][1::2] == 0)


def test_fresh_models_chunked_equals_monolithic(la):
    rng = np.random.default_rng(11)
    for t in range(20):
        n, p = int(rng.integers(20, 300)), int(rng.integers(2, 33))
        X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
        y = (rng.random(n) < 0.5).astype(float)
        dtype = ("float32", "float64")[t % 2]
        m = la.LogReg(X, y, np.full(p, 2.0), dtype=dtype)
        k = la.nutsKernel(m.lpost, m.glp, eps=0.05, dmm=1.0, max_depth=6)
        q0 = 0.1 * rng.standard_normal((96, p))
        full, dfull, _ = run(la, k, q0, 6, seed=t)
        cs = la.ChainSet(k, q0, seed=t)
        parts = np.concatenate([cs.advance(2, 1).to_host(), cs.advance(4, 1).to_host()])
        assert np.array_equal(full, parts), (t, n, p, dtype)
        assert np.all(np.abs(dfull) >= 1)


def test_planner_reports_the_nuts_variant(la, models, pima):
    from logreg_amd import _lib
    m = models["float32"]
    opts = _lib.RunOpts(n_chains=4096, mode=_lib.MODE_AUTO)
    mode, group, rows = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(m._L.lr_plan_run(m.handle, 4, C.byref(opts), C.byref(mode), C.byref(group), C.byref(rows)))
    assert (mode.value, group.value) == (_lib.MODE_LDS, 16)
    k = kern(la, m)
    assert la.ChainSet(k, np.zeros(8), seed=1).plan() == {"mode": "lds", "group": 16, "rows_per_lane": 0}
    rng = np.random.default_rng(0)
    wide = la.LogReg(rng.standard_normal((100, 40)), (rng.random(100) < 0.5).astype(float), 1.0)
    with pytest.raises(la.LogregHipError, match="p = 40 > 32"):
        la.mcmc(np.zeros(40), la.nutsKernel(wide.lpost, wide.glp), iters=1, verb=False)
    tall = la.LogReg(rng.standard_normal((20000, 8)), (rng.random(20000) < 0.5).astype(float), 1.0)
    with pytest.raises(la.LogregHipError, match="beyond"):
        la.mcmc(np.zeros(8), la.nutsKernel(tall.lpost, tall.glp), iters=1, verb=False)


@pytest.fixture(scope="module")
def kernel_vs_reference(la):
    """nr.GPU_F64_CASES on the float64 kernel, the reference and the double, the last two from the kernel's own inputs"""
    import twin_nuts
    from oracle.oracle import OracleModel
    res = []
    for case in nr.GPU_F64_CASES:
        X, y, ps = nr.synthetic_model(case.p, case.n, 100 + case.p)
        dmm, q0 = nr.case_metric_and_start(case)
        steps = nr.run_stepwise(la, la.LogReg(X, y, ps, dtype="float64"), q0, case.K, case.eps, dmm, case.max_depth, case.seed,
                                case.chain_offset, case.iter_offset)
        om = OracleModel(X, y, ps)
        refs = nr.reference_steps(om.lpost, om.glp, steps, case.eps, dmm, case.max_depth, case.seed, case.chain_offset, case.iter_offset)
        res.append([case, steps, refs, None])
    twin_nuts.install()
    try:
        for r in res:
            case = r[0]
            X, y, ps = nr.synthetic_model(case.p, case.n, 100 + case.p)
            dmm, q0 = nr.case_metric_and_start(case)
            r[3] = nr.run_stepwise(la, la.LogReg(X, y, ps, dtype="float64"), q0, case.K, case.eps, dmm, case.max_depth, case.seed,
                                   case.chain_offset, case.iter_offset, forced=r[1])
    finally:
        twin_nuts.uninstall()
    return res


def test_float64_kernel_equals_the_reference_at_every_width(kernel_vs_reference):
    """Teacher-forced, as tests/test_nuts_reference_cpu.py compares the double: signed depth, leaf count and flags equal, state and
    acceptance statistic within nr.F64_TOL (10 x the deviation measured between the double and the reference on the CPU; the kernel's
    row sums are a third summation order).  A transition is left out only below a reference margin of 1e-9, at most 1 in 1000.
    The cases must reach depth 7 and beyond in every width class (the second leaf-uniform block, deep checkpoints with two
    coordinates per lane) and every stop reason but 'check 2 / 3 only', which the CPU module counts."""
    n = skipped = 0
    worst, mism = 0.0, []
    cnt, deep = collections.Counter(), collections.Counter()
    for case, steps, refs, _ in kernel_vs_reference:
        cn, cs, cm, cw = nr.compare(steps, refs, nr.MIN_MARGIN)
        n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
        mism += [f"{case}: {m}" for m in cm]
        P = 4 if case.p <= 4 else 8 if case.p <= 8 else 16 if case.p <= 16 else 32
        for row in refs:
            for r in row:
                cnt[r.reason] += 1
                deep[P] += abs(r.depth) >= 7
    print(f"kernel vs reference: {n} transitions, {skipped} skipped, largest relative deviation {worst:.3g};", dict(cnt),
          "depth >= 7 per padded width:", dict(deep))
    assert not mism, "\n".join(mism[:20])
    assert skipped <= n / 1000
    assert worst <= nr.F64_TOL
    assert all(deep[P] >= 10 for P in (4, 8, 16, 32)), dict(deep)
    for reason in (nr.DIVERGENCE, nr.SUBTREE, nr.TREE):
        assert cnt[reason] >= 20, dict(cnt)
    assert {c.p for c, _, _, _ in kernel_vs_reference} == {3, 4, 5, 8, 9, 16, 17, 31, 32}
    assert {c.C for c, _, _, _ in kernel_vs_reference} == {1, 3, 65, 257}


def test_float64_kernel_equals_the_double_at_every_width(kernel_vs_reference):
    """test_step_parity_with_the_test_double's assertions at the other widths, from the same inputs: depths and counters equal, states
    to 1e-7 relative."""
    for case, steps, _, twin in kernel_vs_reference:
        for k, (g, t) in enumerate(zip(steps, twin)):
            for f in ("depth", "n_leapfrog", "divergent", "max_depth_hits"):
                assert np.array_equal(g[f], t[f]), (case, k, f, np.argwhere(g[f] != t[f])[:10].tolist())
            np.testing.assert_allclose(g["x_out"], t["x_out"], rtol=1e-7, atol=1e-12, err_msg=str((case, k)))
            np.testing.assert_allclose(g["accept_stat_sum"], t["accept_stat_sum"], rtol=1e-7, err_msg=str((case, k)))


def test_float32_kernel_equals_the_float64_reference_beyond_the_margin(la):
    """The float32 kernel teacher-forced against the float64 reference on the float32-rounded data and state.  Where the reference's
    margin exceeds nr.F32_TAU the signed depth, leaf count and flags are equal and the state and acceptance statistic agree to
    nr.F32_STATE_TOL.  Neither number comes from the kernel: they are 8 x what the reference's NumPy-float32 mode showed against its
    float64 mode on the CPU (tests/test_nuts_reference_cpu.py, profiles/r8_nuts_reference.txt); the kernel's summation order is a third
    one with an error of that size.  At most 10 % of the transitions fall below the margin."""
    from oracle.oracle import OracleModel
    n = skipped = 0
    worst, mism = 0.0, []
    for case in nr.F32_CASES:
        X, y, ps, dmm, q0 = nr.float32_problem(case)
        steps = nr.run_stepwise(la, la.LogReg(X, y, ps, dtype="float32"), q0, case.K, case.eps, dmm, case.max_depth, case.seed,
                                case.chain_offset, case.iter_offset)
        assert steps[0]["x_out"].dtype == np.float32
        om = OracleModel(X, y, ps)
        refs = nr.reference_steps(om.lpost, om.glp, steps, case.eps, dmm, case.max_depth, case.seed, case.chain_offset, case.iter_offset)
        cn, cs, cm, cw = nr.compare(steps, refs, nr.F32_TAU)
        n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
        mism += [f"{case}: {m}" for m in cm]
    print(f"float32 kernel vs float64 reference: {n} transitions, {skipped} below the margin {nr.F32_TAU:g}, largest relative deviation {worst:.3g}")
    assert not mism, "\n".join(mism[:20])
    assert skipped <= 0.10 * n
    assert worst <= nr.F32_STATE_TOL


def test_shifted_shards_with_mixed_neighbours_are_bit_exact(la, models, map_beta):
    """A chain's result depends neither on the three chains that share its wave nor on its row in the wave.  The planned run of
    test_bit_exact_rerun_chunks_shards_and_second_build with the chains mixed inside every wave -- non-finite starts (they finish at
    leaf 0), starts far in the tail, ordinary ones -- and shards whose first chain is 1, 2, 3 (mod 4) with odd lengths: every chain
    moves to another row and gets other neighbours.  Samples, depths and counters are compared as bytes."""
    rng = np.random.default_rng(6)
    C = 1000
    sd = np.array([1.73, 0.065, 0.0068, 0.018, 0.023, 0.043, 0.55, 0.022])
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((C, 8))
    kind = rng.integers(0, 3, C)  # 0 ordinary, 1 non-finite, 2 tail: mixed within the waves
    q0[kind == 1, 3] = np.nan
    q0[kind == 2] = map_beta + 6.0 * sd * rng.standard_normal((int((kind == 2).sum()), 8))
    fields = ("n_leapfrog", "depth_sum", "accept_stat_sum", "divergent", "max_depth_hits")
    for dtype in ("float32", "float64"):
        k = kern(la, models[dtype], max_depth=8)
        full, dfull, cs = run(la, k, q0, 12, thin=2)
        cfull = cs.get_counters()
        assert np.all(dfull[:, kind == 1] == -1) and np.all(np.abs(dfull[:, kind != 1]) >= 1)
        assert len({tuple(kind[w:w + 4]) for w in range(0, C, 4)}) > 20  # the waves really are mixed
        for lo, hi in ((1, 78), (301, 432), (502, 757), (663, 1000), (998, 999)):
            assert lo % 4 in (1, 2, 3) and (hi - lo) % 2 == 1
            sh, dsh, css = run(la, k, q0[lo:hi], 12, thin=2, chain_offset=lo, plan_chains=C, plan_first=0)
            assert sh.tobytes() == full[:, lo:hi].tobytes(), (dtype, lo, hi)
            assert dsh.tobytes() == dfull[:, lo:hi].tobytes(), (dtype, lo, hi)
            csh = css.get_counters()
            for f in fields:
                assert np.asarray(csh[f]).tobytes() == np.ascontiguousarray(cfull[f][lo:hi]).tobytes(), (dtype, lo, hi, f)
