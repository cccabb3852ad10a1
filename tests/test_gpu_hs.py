"""The fused horseshoe Polya-Gamma Gibbs kernel (logreg_amd/csrc/lr_hs.h, include/logreg_hip_hs.h) on the MI355X: the hyper-step and the
sweep against the independent NumPy reference (tests/hs_reference.py) in both dtypes, the empty shrink set against lr_run_pg byte for
byte, the posterior of a small model against an importance-sampling estimate that shares no Gibbs code (tests/golden/
hs_small_posterior.json), bit exactness of reruns, chunks, shards, save / resume and the second build, fresh models, the accumulators
on a summary-only run, extreme starts."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import hs_reference as hr
import pg_reference as pr

pytestmark = pytest.mark.gpu

HYPER_TOL = 1e-12  # every quantity is a sum of positive terms of the same inputs: ~40 operations of <= 2 ulp, two decades for libm


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
    """the float64 reference sweep of a case under hr.case_prior (computed once, shared): on the data as given, or rounded to float32 first"""
    key = (case, rounded)
    if key not in _ref_cache:
        X, y, ps, st = pr.make_case(case)
        if rounded:
            X, st = X.astype(np.float32).astype(np.float64), st.astype(np.float32).astype(np.float64)
        mask, tau0, hyper = hr.case_prior(case)
        _ref_cache[key] = hr.sweep(pr.signed_rows(X, y), ps, st, hyper, mask, tau0, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
    return _ref_cache[key]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_hyper_step_against_the_reference(la, dtype):
    """1. lr_hs_hyper at the nine widths, hyper-states log-uniform over 10^+-6 with one chain at the clamp: within 1e-12, clamp counts equal"""
    worst, clamps = 0.0, 0
    for case in pr.GPU_CASES:
        rng = np.random.default_rng(case.p * 31 + case.C)
        mask, tau0, hyper = hr.random_mask(rng, case.p), 0.37, hr.random_hyper(rng, case.C, case.p)
        st = pr.make_case(case)[3].astype(dtype)
        got, cn = hr.library_hyper(la, case, dtype, mask, tau0, hyper, states=st)
        ref, rcn = hr.hyper_step(st.astype(np.float64), hyper, mask, tau0, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
        dev = hr.hyper_dev(got, ref)
        print(case, f"hyper-step deviation {dev:.3g}, clamps {int(cn.sum())}")
        assert np.array_equal(cn, rcn), case
        worst, clamps = max(worst, dev), clamps + int(cn.sum())
    print(f"{dtype} hyper-step: largest relative deviation {worst:.4g} (bound {HYPER_TOL:g}), {clamps} clamps")
    assert worst <= HYPER_TOL and clamps > 0


def test_empty_shrink_set_equals_pg_byte_for_byte(la, models, map_beta):
    """2. lr_run_hs accepts the empty set (include/logreg_hip_hs.h): states, out and the three shared counters are lr_run_pg's bytes"""
    from logreg_amd import _lib
    L = _lib.load_hs()
    _lib.bind_pg(L)
    rng = np.random.default_rng(5)
    C = 1000
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((C, 8))
    q0[5::17] *= 60.0          # far-tail starts: |psi| in the hundreds
    q0[7::29, 2] = np.nan      # non-finite starts
    q0[11::31, 0] = np.inf
    for dtype, m in models.items():
        opts = _lib.RunOpts(n_chains=C, chain_offset=3, thin=2, iters=12, iter_offset=5, seed=7, group=0, mode=_lib.MODE_AUTO, on_device=0)
        a, b = (np.ascontiguousarray(q0, dtype=m.np_dtype).copy() for _ in range(2))
        oa, ob = (np.zeros((12, C, 8), dtype=m.np_dtype) for _ in range(2))
        ca, cb = np.zeros(C, dtype=la.kernels.PG_COUNTERS), np.zeros(C, dtype=la.kernels.HS_COUNTERS)
        keep, prior = hr._prior(np.zeros(8, bool), 1.0)
        h = 10.0 ** rng.uniform(-3, 3, (C, 18))  # (never read by the model: s_j = 0)
        assert L.lr_run_pg(m.handle, a.ctypes.data, ctypes.byref(opts), oa.ctypes.data, ca.ctypes.data) == 0, L.lr_last_error()
        assert L.lr_run_hs(m.handle, ctypes.byref(prior), b.ctypes.data, h.ctypes.data, ctypes.byref(opts), ob.ctypes.data, None, cb.ctypes.data) == 0, L.lr_last_error()
        assert a.tobytes() == b.tobytes() and oa.tobytes() == ob.tobytes(), dtype
        assert all(np.array_equal(ca[f], cb[f]) for f in ("proposals", "series_terms", "skipped")), dtype
        assert ca["skipped"][7] == 24 and ca["skipped"][0] == 0 and np.all(np.isfinite(h))


def test_sweep_float64_against_the_reference(la):
    """3. one sweep at the nine widths: beta within pr.F64_TOL, the Polya-Gamma counters equal, the hyper-state within 1e-12 of the
    reference's hyper-step at the GPU's own new beta"""
    worst_b = worst_h = 0.0
    for case in pr.GPU_CASES:
        ref = reference(case, False)
        mask, tau0, hyper = hr.case_prior(case)
        st, h, cn = hr.library_sweep(la, case, "float64", mask, tau0, hyper)
        assert np.array_equal(cn["proposals"], ref.proposals) and np.array_equal(cn["series_terms"], ref.terms) and not cn["skipped"].any(), case
        hh, hcn = hr.hyper_step(st, hyper, mask, tau0, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
        d_b, d_h = pr.rel_dev(st, ref.beta), hr.hyper_dev(h, hh)
        print(case, f"state deviation {d_b:.3g}, hyper-state deviation {d_h:.3g}")
        assert np.array_equal(cn["clamped"], hcn), case
        worst_b, worst_h = max(worst_b, d_b), max(worst_h, d_h)
    print(f"float64 sweep: largest relative deviation of the state {worst_b:.4g} (F64_TOL {pr.F64_TOL:g}), of the hyper-state {worst_h:.4g} (bound {HYPER_TOL:g})")
    assert worst_b <= pr.F64_TOL and worst_h <= HYPER_TOL


def test_sweep_float32_against_the_float64_reference(la):
    """3. float32: a chain is compared if all its n draws clear pr.F32_TAU (at most 10 % of the chains are left out: phase 1 is PG's on
    the same states); states within pr.F32_STATE_TOL, counters of the compared chains equal, the hyper-state as in float64"""
    chains = left_out = 0
    worst_b = worst_h = 0.0
    for case in pr.F32_CASES:
        ref = reference(case, True)
        mask, tau0, hyper = hr.case_prior(case)
        st, h, cn = hr.library_sweep(la, case, "float32", mask, tau0, hyper)
        keep = np.all(ref.margin >= pr.F32_TAU, axis=1)
        chains, left_out = chains + case.C, left_out + int((~keep).sum())
        assert not cn["skipped"].any()
        assert np.array_equal(cn["proposals"][keep], ref.proposals[keep]) and np.array_equal(cn["series_terms"][keep], ref.terms[keep]), case
        hh, hcn = hr.hyper_step(st.astype(np.float64), hyper, mask, tau0, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
        d_b, d_h = pr.rel_dev(st[keep], ref.beta[keep]), hr.hyper_dev(h, hh)
        print(case, f"state deviation {d_b:.3g}, hyper-state deviation {d_h:.3g}")
        assert np.array_equal(cn["clamped"], hcn), case
        worst_b, worst_h = max(worst_b, d_b), max(worst_h, d_h)
    print(f"float32 sweep: {chains} chains, {left_out} left out, largest relative deviation of the state {worst_b:.4g} (F32_STATE_TOL {pr.F32_STATE_TOL:g}), "
          f"of the hyper-state {worst_h:.4g}")
    assert left_out <= 0.10 * chains
    assert worst_b <= pr.F32_STATE_TOL and worst_h <= HYPER_TOL


def _run(la, k, q0, parts, thin, seed=7, resume_dir=None, **kw):
    """a run in `parts` launches (saved and resumed between them with resume_dir) -> (out, scales, hyper, counters) as bytes"""
    cs = la.ChainSet(k, q0, seed=seed, **kw)
    cs.set_hyper(np.concatenate([np.full(8, 0.5), np.full(8, 2.0), [0.04, 3.0]]))
    outs, scs = [], []
    for i, n in enumerate(parts):
        if resume_dir is not None and i > 0:
            cs = la.ChainSet.resume(k, cs.save(resume_dir / f"part{i}"))
        sc = la.DeviceArray(cs.model.device, (n, cs.C, 9), np.float64)
        outs.append(cs.advance(n, thin, scales=sc).to_host())
        scs.append(sc.to_host())
        sc.free()
    return np.concatenate(outs), np.concatenate(scs), cs.get_hyper(), cs.get_counters()


def test_bit_exact_rerun_chunks_shards_resume_and_second_build(la, models, map_beta, pima, pscale, tmp_path):
    """4. bytes of the states, the hyper-state, scale_out and the counters"""
    import altlib
    rng = np.random.default_rng(5)
    C = 600
    q0 = map_beta + 0.1 * np.abs(map_beta) * rng.standard_normal((C, 8))
    q0[5::17] *= 60.0
    q0[7::29, 2] = np.nan
    mask = np.array([False, True, True, False, True, True, True, True])

    def same(a, b, sl=slice(None)):
        return a[0][:, sl].tobytes() == b[0].tobytes() and a[1][:, sl].tobytes() == b[1].tobytes() and a[2][sl].tobytes() == b[2].tobytes() and a[3][sl].tobytes() == b[3].tobytes()
    for dtype in ("float32", "float64"):
        k = la.hsKernel(models[dtype].lpost, shrink=mask, global_scale=0.2)
        full = _run(la, k, q0, (12,), 2)
        assert same(full, _run(la, k, q0, (12,), 2)), "rerun"
        assert full[3]["skipped"][7] == 24 and full[3]["skipped"][0] == 0 and np.all(np.isfinite(full[1])) and np.all(np.isfinite(full[2]))
        assert np.all(full[1][:, :, [0, 3]] == 1.0) and np.all(full[1][:, 0, 1] != 0.5) and np.all(full[1][:, 7, :8][:, mask] == 0.5)  # (a skipped chain keeps its scales)
        assert same(full, _run(la, k, q0, (5, 7), 2)), "chunks"
        assert same(full, _run(la, k, q0, (5, 7), 2, resume_dir=tmp_path)), "save / resume"
        for lo, n in ((1, 37), (102, 55), (303, 111), (5, 1), (590, 9)):  # shards at odd offsets, odd lengths
            assert same(full, _run(la, k, q0[lo:lo + n], (12,), 2, chain_offset=lo, plan_chains=C, plan_first=0), slice(lo, lo + n)), (dtype, lo, n)
        altlib.install()  # the second build of the same sources
        try:
            m_alt = la.LogReg(*pima, pscale, dtype=dtype)
            alt = _run(la, la.hsKernel(m_alt.lpost, shrink=mask, global_scale=0.2), q0, (12,), 2)
        finally:
            altlib.uninstall()
        assert same(full, alt), "second build"


def test_fresh_models_chunked_equals_monolithic(la):
    """5. twenty random models (n <= 300, p <= 32, dtype, mask)"""
    rng = np.random.default_rng(78)
    for _ in range(20):
        n, p = int(rng.integers(20, 301)), int(rng.integers(2, 33))
        dtype = "float32" if rng.random() < 0.5 else "float64"
        X = rng.standard_normal((n, p))
        X[:, 0] = 1.0
        y = (rng.random(n) < 0.4).astype(np.float64)
        m = la.LogReg(X, y, rng.uniform(0.5, 3.0, p), dtype=dtype)
        mask = rng.random(p) < 0.6
        mask[int(rng.integers(0, p))] = True
        k = la.hsKernel(m.lpost, shrink=mask, global_scale=float(10.0 ** rng.uniform(-2, 0)))
        q0 = 0.3 * rng.standard_normal((int(rng.integers(1, 70)), p))
        seed = int(rng.integers(1, 1 << 30))
        whole, wi = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=seed, return_info=True)
        parts, pi = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=seed, chunk=int(rng.integers(1, 5)), return_info=True)
        assert whole.tobytes() == parts.tobytes() and np.all(np.isfinite(whole)), (n, p, dtype)
        for f in ("hyper", "local_scale2", "global_scale2", "clamped", "proposals"):
            assert wi[f].tobytes() == pi[f].tobytes() and np.all(np.isfinite(wi[f])), (n, p, dtype, f)
        assert np.all(wi["local_scale2"][:, :, ~mask] == 1.0)
        m.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_posterior_on_the_small_model(la, dtype):
    """6. 4096 chains, 100 sweeps dropped, 200 kept: z of every stored quantity against the importance-sampling estimates, |z| < 4.2"""
    fx = load_golden("hs_small_posterior.json")
    X, y = hr.small_model()
    m = la.LogReg(X, y, hr.SMALL_PSCALE, dtype=dtype)
    k = la.hsKernel(m.lpost, shrink=hr.SMALL_MASK, global_scale=hr.SMALL_TAU0)
    cs = la.ChainSet(k, np.zeros((4096, 3)), seed=2025)
    cs.advance(1, 100, keep=False)
    sc = la.DeviceArray(m.device, (200, 4096, 4), np.float64)
    beta = cs.advance(200, 1, scales=sc).to_host()
    scales = sc.to_host()
    info = cs.pg_info()
    zm, zs = hr.z_against_fixture(hr.posterior_quantities(beta, scales[:, :, :3], scales[:, :, 3]), fx, la.summarise)
    print(dtype, "z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2), "clamped", int(info["clamped"].sum()), "skipped", int(info["skipped"].sum()))
    assert info["skipped"].sum() == 0
    assert np.max(np.abs(zm)) < hr.Z_BOUND and np.max(np.abs(zs)) < hr.Z_BOUND
    m.close()


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) if np.asarray(a).dtype.kind in "fc" else np.array_equal(np.asarray(a), np.asarray(b))


def test_accumulators_on_a_summary_only_run(la, models, map_beta):
    """7. one summary_only run with a RankDiagnostics, a PsisLoo and a PredictiveCheck attached equals feeding the kept draws by hand;
    bridge= is refused with the reason"""
    m = models["float32"]
    k = la.hsKernel(m.lpost, global_scale=0.1)
    C, iters = 128, 24
    q0 = np.tile(map_beta, (C, 1))
    groups = (np.arange(m.n) % 3).astype(np.int32)
    kw = dict(thin=1, iters=iters, verb=False, seed=9, chunk=10)
    accs = dict(rank=la.RankDiagnostics(C, 8, iters, "float32"), loo=la.PsisLoo(m, C * iters), check=la.PredictiveCheck(m, groups=groups, seed=21))
    res = la.mcmc(q0, k, summary_only=True, **accs, **kw)
    kept, info = la.mcmc(q0, k, return_info=True, **kw)
    hand = dict(rank=la.RankDiagnostics(C, 8, iters, "float32"), loo=la.PsisLoo(m, C * iters), check=la.PredictiveCheck(m, groups=groups, seed=21))
    for name, acc in hand.items():
        acc.update(kept)
        if name != "check":
            assert _same(dict(res[name]), dict(acc.result())), name
    # the predictive check: its integer tables are exact; its four deviance moments are float sums in the order of the chunks
    ta, tb = accs["check"].tables(), hand["check"].tables()
    assert ta["n_draws"] == tb["n_draws"] == C * iters and all(ta[t].tobytes() == tb[t].tobytes() for t in ("hist", "row_ones", "counts", "t_obs", "n_g"))
    np.testing.assert_allclose(ta["moments"], tb["moments"], rtol=1e-12)
    assert accs["loo"].table().tobytes() == hand["loo"].table().tobytes() and accs["rank"].table().tobytes() == hand["rank"].table().tobytes()
    assert np.array_equal(res["hyper"], info["hyper"]) and np.array_equal(res["state"], info["state"]) and res["skipped"].sum() == 0 and res["accept_rate"] == 1.0
    np.testing.assert_allclose(res["mean"], kept.astype(np.float64).mean(axis=(0, 1)), rtol=1e-5)
    br = la.Bridge(m, map_beta, 0.01 * np.eye(8), C * iters)
    with pytest.raises(ValueError, match="Gaussian prior"):
        la.mcmc(q0, k, summary_only=True, bridge=br, **kw)
    br.close()
    accs["rank"].free()
    hand["rank"].free()
    for name in ("loo", "check"):
        accs[name].close()
        hand[name].close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_extreme_starts_stay_finite(la, dtype):
    """8. |psi| up to 700, lambda^2 = 1e-90 and tau^2 = 1e90 (and the reverse): states and hyper-state stay finite, the counters are reported"""
    case = pr.GPU_CASES[8]
    X, y, ps, st = pr.make_case(case)
    st = st * (700.0 / np.max(np.abs(st @ pr.signed_rows(X, y).T)))
    m = la.LogReg(X, y, ps, dtype=dtype)
    k = la.hsKernel(m.lpost, global_scale=1.0)
    cs = la.ChainSet(k, st, seed=3)
    h = hr.default_hyper(case.C, case.p, 1.0)
    h[:, :case.p], h[:, 2 * case.p] = 1e-90, 1e90
    h[1::2, :case.p], h[1::2, 2 * case.p] = 1e90, 1e-90
    h[2::5, case.p:2 * case.p], h[2::5, 2 * case.p + 1] = 1e-100, 1e100
    cs.set_hyper(h)
    out = cs.advance(10, 1).to_host()
    hyper, info = cs.get_hyper(), cs.pg_info()
    print(dtype, "skipped", int(info["skipped"].sum()), "clamped", int(info["clamped"].sum()), "of", case.C * 10, "sweeps; hyper-state in", hyper.min(), hyper.max())
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(hyper)) and np.all(hyper >= 1e-100) and np.all(hyper <= 1e100)
    assert np.all(info["skipped"] < 10)  # no chain is pinned on the skip rule
    m.close()
