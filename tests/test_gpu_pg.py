"""The fused Polya-Gamma Gibbs kernel (logreg_amd/csrc/lr_pg.h, include/logreg_hip_pg.h) on the MI355X: the draw omega by omega and
the sweep state by state against the independent NumPy reference (tests/pg_reference.py) and the CPU test double, in both dtypes with
the tolerances fixed on the CPU (tests/test_pg_cpu.py); the posterior against the reference's; bit exactness of reruns, chunks, shards
and the second build; fresh models; the planner; the accumulators on a summary-only run."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import pg_reference as pr

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


_ref_cache = {}


def reference(case, rounded):
    """the float64 reference sweep of a case (computed once, shared): on the data as given, or rounded to float32 first"""
    key = (case, rounded)
    if key not in _ref_cache:
        X, y, ps, st = pr.make_case(case)
        if rounded:
            X, st = X.astype(np.float32).astype(np.float64), st.astype(np.float32).astype(np.float64)
        _ref_cache[key] = pr.sweep(pr.signed_rows(X, y), ps, st, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
    return _ref_cache[key]


def library_sweep(la, case, dtype, states=None, omega_only=False):
    """one sweep of the case through the C ABI of whatever library is loaded: -> (omega [C, n], new states [C, p], counters [C])"""
    from logreg_amd import _lib
    L = _lib.load_pg()
    X, y, ps, st = pr.make_case(case)
    m = la.LogReg(X, y, ps, dtype=dtype)
    st = np.ascontiguousarray(st if states is None else states, dtype=m.np_dtype)
    opts = _lib.RunOpts(n_chains=case.C, chain_offset=case.chain_offset, thin=1, iters=1, iter_offset=case.iter_offset, seed=case.seed, group=0,
                        mode=_lib.MODE_AUTO, on_device=0)
    om = np.empty((case.C, case.n), dtype=m.np_dtype)
    before = st.copy()
    assert L.lr_pg_omega(m.handle, st.ctypes.data, ctypes.byref(opts), om.ctypes.data) == 0, L.lr_last_error()
    assert st.tobytes() == before.tobytes()  # the state is not moved
    cn = np.zeros(case.C, dtype=la.kernels.PG_COUNTERS)
    if not omega_only:
        assert L.lr_run_pg(m.handle, st.ctypes.data, ctypes.byref(opts), None, cn.ctypes.data) == 0, L.lr_last_error()
    m.close()
    return om, st, cn


def z_scores(summ, ref):
    zm = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    se_sd = summ["sd"] / np.sqrt(2 * summ["ess"])
    zs = (summ["sd"] - np.array(ref["sd"])) / np.sqrt(se_sd ** 2 + np.array(ref["se_sd"]) ** 2)
    return zm, zs


def test_omega_float64_against_the_reference(la):
    """lr_pg_omega at the nine widths: omega within F64_TOL wherever the reference's margin is >= 1e-9, at most 1 draw in 1000 left out."""
    total = left_out = 0
    worst = 0.0
    for case in pr.GPU_CASES:
        ref = reference(case, False)
        om, _, _ = library_sweep(la, case, "float64", omega_only=True)
        keep = ref.margin >= 1e-9
        total, left_out = total + keep.size, left_out + int((~keep).sum())
        dev = pr.omega_dev(om[keep], ref.omega[keep])
        worst = max(worst, dev)
        print(case, f"omega deviation {dev:.3g}")
        assert np.all(np.isfinite(om)) and np.all(om > 0)
    print(f"float64 omega: {total} draws, {left_out} below the margin, largest relative deviation {worst:.4g} (F64_TOL {pr.F64_TOL:g})")
    assert left_out <= total / 1000
    assert worst <= pr.F64_TOL


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_omega_is_finite_and_positive_at_extreme_psi(la, dtype):
    """states scaled so that |psi| reaches 700 (exp(2 z) overflows float32 from |psi| = 88 and float64 from 709)"""
    for case in (pr.GPU_CASES[3], pr.GPU_CASES[8]):
        X, y, ps, st = pr.make_case(case)
        psi = st @ pr.signed_rows(X, y).T
        st = st * (700.0 / np.max(np.abs(psi)))
        om, _, _ = library_sweep(la, case, dtype, states=st, omega_only=True)
        hi = np.abs((st.astype(om.dtype).astype(np.float64)) @ pr.signed_rows(X, y).T)
        print(dtype, case, "max |psi|", hi.max(), "share of |psi| > 88:", np.mean(hi > 88), "omega in", om.min(), om.max())
        assert hi.max() > 690 and np.all(np.isfinite(om)) and np.all(om > 0)
        big = hi > 400  # E omega = tanh(psi / 2) / (2 psi) and the sd is far below it there
        assert np.all(np.abs(om[big] * 2 * hi[big] - 1) < 0.5)


def test_omega_float32_against_the_float64_reference(la):
    """the float32 kernel against the float64 reference on float32-rounded data: within F32_OMEGA_TOL wherever the reference's margin
    is >= F32_TAU (both fixed on the CPU from the reference's own two modes); at most 1 % of the draws below the margin"""
    total = left_out = 0
    worst = 0.0
    for case in pr.GPU_CASES:
        ref = reference(case, True)
        om, _, _ = library_sweep(la, case, "float32", omega_only=True)
        keep = ref.margin >= pr.F32_TAU
        total, left_out = total + keep.size, left_out + int((~keep).sum())
        dev = pr.omega_dev(om[keep], ref.omega[keep])
        worst = max(worst, dev)
        print(case, f"omega deviation {dev:.3g}")
    print(f"float32 omega: {total} draws, {left_out} below the margin, largest relative deviation {worst:.4g} (F32_OMEGA_TOL {pr.F32_OMEGA_TOL:g})")
    assert left_out <= total / 100
    assert worst <= pr.F32_OMEGA_TOL


def test_transition_float64_against_the_reference_and_the_double(la):
    """states within F64_TOL of the reference and of the double, counters equal to both"""
    import twin_pg
    gpu = {case: library_sweep(la, case, "float64") for case in pr.GPU_CASES}
    twin_pg.install()
    try:
        dbl = {case: library_sweep(la, case, "float64") for case in pr.GPU_CASES}
    finally:
        twin_pg.uninstall()
    worst_ref = worst_dbl = 0.0
    for case in pr.GPU_CASES:
        ref = reference(case, False)
        _, st, cn = gpu[case]
        _, st_d, cn_d = dbl[case]
        assert np.array_equal(cn["proposals"], ref.proposals) and np.array_equal(cn["series_terms"], ref.terms) and not cn["skipped"].any(), case
        assert cn.tobytes() == cn_d.tobytes(), case
        d_ref, d_dbl = pr.rel_dev(st, ref.beta), pr.rel_dev(st, st_d)
        print(case, f"state deviation from the reference {d_ref:.3g}, from the double {d_dbl:.3g}")
        worst_ref, worst_dbl = max(worst_ref, d_ref), max(worst_dbl, d_dbl)
    print(f"float64 transition: largest relative deviation from the reference {worst_ref:.4g}, from the double {worst_dbl:.4g} (F64_TOL {pr.F64_TOL:g})")
    assert worst_ref <= pr.F64_TOL and worst_dbl <= pr.F64_TOL


def test_transition_float32_against_the_float64_reference(la):
    """a chain is compared if all its n draws clear F32_TAU (n <= 40: at most 10 % of the chains are left out); states within F32_STATE_TOL"""
    chains = left_out = 0
    worst = 0.0
    for case in pr.F32_CASES:
        ref = reference(case, True)
        _, st, cn = library_sweep(la, case, "float32")
        keep = np.all(ref.margin >= pr.F32_TAU, axis=1)
        chains, left_out = chains + case.C, left_out + int((~keep).sum())
        dev = pr.rel_dev(st[keep], ref.beta[keep])
        worst = max(worst, dev)
        print(case, f"state deviation {dev:.3g}")
        assert not cn["skipped"].any()
    print(f"float32 transition: {chains} chains, {left_out} left out, largest relative deviation {worst:.4g} (F32_STATE_TOL {pr.F32_STATE_TOL:g})")
    assert left_out <= 0.10 * chains
    assert worst <= pr.F32_STATE_TOL


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_posterior_matches_the_reference(la, models, map_beta, dtype):
    ref = load_golden("posterior_hmc.json")["pooled"]
    C = 4096
    cs = la.ChainSet(la.pgKernel(models[dtype].lpost), np.tile(map_beta, (C, 1)), seed=2024)
    cs.advance(1, 50, keep=False)
    samples = cs.advance(100, 1).to_host()
    info = cs.pg_info()
    zm, zs = z_scores(la.summarise(samples, max_chains=128), ref)
    print(dtype, "z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2), "proposals per draw", info["proposals_per_draw"].mean(), "series terms per draw",
          info["series_terms_per_draw"].mean())
    assert info["skipped"].sum() == 0
    assert np.max(np.abs(zm)) < 4.2 and np.max(np.abs(zs)) < 4.2


def _run(la, k, q0, iters, thin, seed=7, **kw):
    cs = la.ChainSet(k, q0, seed=seed, **kw)
    out = cs.advance(iters, thin).to_host()
    return out, cs.get_counters()


def test_bit_exact_rerun_chunks_shards_and_second_build(la, models, map_beta, pima, pscale):
    import altlib
    rng = np.random.default_rng(5)
    C = 1000
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((C, 8))
    q0[5::17] *= 60.0          # far-tail starts: |psi| in the hundreds
    q0[7::29, 2] = np.nan      # non-finite starts
    q0[11::31, 0] = np.inf
    for dtype in ("float32", "float64"):
        k = la.pgKernel(models[dtype].lpost)
        full, cfull = _run(la, k, q0, 12, 2)
        again, cagain = _run(la, k, q0, 12, 2)
        assert full.tobytes() == again.tobytes() and cfull.tobytes() == cagain.tobytes()
        assert cfull["skipped"][7] == 24 and cfull["skipped"][11] == 24 and cfull["skipped"][0] == 0 and np.all(np.isfinite(full[:, 5]))
        cs = la.ChainSet(k, q0, seed=7)
        parts = [cs.advance(n, 2).to_host() for n in (5, 7)]  # chunked: iter_offset
        assert np.concatenate(parts).tobytes() == full.tobytes() and cs.get_counters().tobytes() == cfull.tobytes()
        for lo, n in ((1, 37), (102, 55), (303, 111), (5, 1), (990, 9)):  # shards from chain ids 1, 2, 3, 1, 2 (mod 4), odd lengths
            sh, csh = _run(la, k, q0[lo:lo + n], 12, 2, chain_offset=lo, plan_chains=C, plan_first=0)
            assert sh.tobytes() == full[:, lo:lo + n].tobytes() and csh.tobytes() == cfull[lo:lo + n].tobytes(), (dtype, lo, n)
        altlib.install()  # the second build of the same sources: bytes compared
        try:
            m_alt = la.LogReg(*pima, pscale, dtype=dtype)
            alt, calt = _run(la, la.pgKernel(m_alt.lpost), q0, 12, 2)
        finally:
            altlib.uninstall()
        assert full.tobytes() == alt.tobytes() and cfull.tobytes() == calt.tobytes()


def test_fresh_models_chunked_equals_monolithic(la):
    rng = np.random.default_rng(77)
    for _ in range(20):
        n, p = int(rng.integers(20, 301)), int(rng.integers(2, 33))
        dtype = "float32" if rng.random() < 0.5 else "float64"
        X = rng.standard_normal((n, p))
        X[:, 0] = 1.0
        y = (rng.random(n) < 0.4).astype(np.float64)
        m = la.LogReg(X, y, rng.uniform(0.5, 3.0, p), dtype=dtype)
        k = la.pgKernel(m.lpost)
        q0 = 0.3 * rng.standard_normal((int(rng.integers(1, 70)), p))
        seed = int(rng.integers(1, 1 << 30))
        whole = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=seed)
        parts = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=seed, chunk=int(rng.integers(1, 5)))
        assert whole.tobytes() == parts.tobytes() and np.all(np.isfinite(whole)), (n, p, dtype)
        m.close()


def test_planner(la, models):
    from logreg_amd import _lib
    for m in models.values():
        plan = la.ChainSet(la.pgKernel(m.lpost), np.zeros((64, 8)), seed=1).plan()
        assert plan["mode"] == "lds" and plan["group"] == 16 and "tail" not in plan
    rng = np.random.default_rng(2)
    for n, p, word in ((50, 40, "p = 40 > 32"), (20000, 8, "bytes of LDS")):
        X = rng.standard_normal((n, p))
        m = la.LogReg(X, (rng.random(n) < 0.5).astype(np.float64), np.ones(p), dtype="float32")
        with pytest.raises(_lib.LogregHipError, match=word):
            la.ChainSet(la.pgKernel(m.lpost), np.zeros((64, p)), seed=1).plan()
        with pytest.raises(_lib.LogregHipError, match=word):
            la.mcmc(np.zeros((64, p)), la.pgKernel(m.lpost), thin=1, iters=2, verb=False, seed=1)
        m.close()


def test_accumulators_on_a_summary_only_run(la, models, map_beta):
    """one summary_only run with an Autocorr and a Covariance attached equals feeding the kept draws by hand"""
    m = models["float32"]
    k = la.pgKernel(m.lpost)
    C, iters = 256, 40
    q0 = np.tile(map_beta, (C, 1))
    sd = np.array([1.73, 0.065, 0.0068, 0.018, 0.023, 0.043, 0.55, 0.022])
    center, scale = la.covariance_scaling(map_beta, sd)
    ac, cv = la.Autocorr(C, 8, "float32", max_lag=15), la.Covariance(C, 8, "float32", center, scale)
    res = la.mcmc(q0, k, thin=1, iters=iters, verb=False, seed=9, summary_only=True, autocorr=ac, covariance=cv, chunk=16)
    kept = la.mcmc(q0, k, thin=1, iters=iters, verb=False, seed=9)
    ac2, cv2 = la.Autocorr(C, 8, "float32", max_lag=15), la.Covariance(C, 8, "float32", center, scale)
    ac2.update(kept)
    cv2.update(kept)
    a, b = res["autocorr"], ac2.result()
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["ess"], b["ess"])
    c, d = res["covariance"], cv2.result()
    assert np.array_equal(c["cov"], d["cov"]) and np.array_equal(c["mean"], d["mean"])
    np.testing.assert_allclose(res["mean"], kept.astype(np.float64).mean(axis=(0, 1)), rtol=1e-5)
    assert res["skipped"].sum() == 0 and res["accept_rate"] == 1.0
    print("min ESS per kept sweep", (a["ess"] / (C * iters)).min(), "max", (a["ess"] / (C * iters)).max())
