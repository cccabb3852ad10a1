"""The horseshoe Polya-Gamma Gibbs sampler (include/logreg_hip_hs.h) -- everything that can be checked without a GPU: the NumPy reference
(tests/hs_reference.py) against an importance-sampling estimate of the posterior that shares no Gibbs code with it
(tests/golden/hs_small_posterior.json), the CPU test double (tests/host/lr_cpu_twin_hs.c) against the reference hyper-step by hyper-step
and sweep by sweep, the Python face (hsKernel, ChainSet, mcmc) on the double, the ABI tables and exports of both builds, the kernels'
gates, and the host side of the run under AddressSanitizer and UBSan as a stand-alone program (tests/host/hs_harness.cpp)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import host_build
import hs_reference as hr
import pg_reference as pr
import twin_hs

WANT = ["lr_hs_hyper", "lr_run_hs"]
HYPER_TOL = 1e-12  # the issue's bound on the hyper-step: ~40 operations of <= 2 ulp on sums of positive terms, two decades for libm


@pytest.fixture(scope="module", autouse=True)
def _hs_twin():
    twin_hs.install()
    yield
    twin_hs.uninstall()


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def test_the_fixture_is_its_generators():
    fx = load_golden("hs_small_posterior.json")
    X, y = hr.small_model()
    assert np.array_equal(np.array(fx["X"]), X) and np.array_equal(np.array(fx["y"]), y) and X.shape == (12, 3)
    assert fx["pscale"] == [3.0, 2.0, 2.0] and fx["shrink"] == [False, True, True] and fx["global_scale"] == 1.0 and fx["draws"] >= 2_000_000
    assert fx["names"] == ["beta_0", "beta_1", "beta_2", "kappa_1", "kappa_2", "log_tau2"]
    assert len(fx["mean"]) == len(fx["mean_mcse"]) == 6 and len(fx["sd"]) == len(fx["sd_mcse"]) == 3
    assert 0 < y.sum() < 12 and os.path.exists(os.path.join(REPO, "tests", "golden", "make_hs_small_posterior.py"))


def test_reference_sampler_meets_the_gpu_criterion_on_the_small_model(la):
    """The target check: 4096 chains of the NumPy reference, 100 sweeps dropped and 200 kept, against the importance-sampling estimates --
    the criterion of tests/test_gpu_hs.py::test_posterior_on_the_small_model, so that bound is known to be attainable."""
    fx = load_golden("hs_small_posterior.json")
    X, y = hr.small_model()
    C = 4096
    b, l2, t2 = hr.run_small(pr.signed_rows(X, y), hr.SMALL_PSCALE, np.zeros((C, 3)), hr.default_hyper(C, 3, hr.SMALL_TAU0), hr.SMALL_MASK, hr.SMALL_TAU0, 31, 200, drop=100)
    zm, zs = hr.z_against_fixture(hr.posterior_quantities(b, l2, t2), fx, la.summarise)
    print("z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2))
    assert np.max(np.abs(zm)) < hr.Z_BOUND and np.max(np.abs(zs)) < hr.Z_BOUND


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_hyper_step_of_the_double_equals_the_reference(la, dtype):
    """lr_hs_hyper of the double over pr.CPU_CASES, hyper-states log-uniform over 10^+-6 with one chain at the clamp: within 1e-12,
    clamp counts equal"""
    worst, clamps = 0.0, 0
    for case in pr.CPU_CASES:
        rng = np.random.default_rng(case.p * 31 + case.C)
        mask, tau0, hyper = hr.random_mask(rng, case.p), 0.37, hr.random_hyper(rng, case.C, case.p)
        _, _, _, st = pr.make_case(case)
        st = st.astype(dtype)
        got, cn = hr.library_hyper(la, case, dtype, mask, tau0, hyper, states=st)
        ref, rcn = hr.hyper_step(st.astype(np.float64), hyper, mask, tau0, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
        assert np.array_equal(cn, rcn), case
        worst, clamps = max(worst, hr.hyper_dev(got, ref)), clamps + int(cn.sum())
        assert np.array_equal(got[:, :case.p][:, ~mask], hyper[:, :case.p][:, ~mask])  # unshrunk entries are carried
    print(f"{dtype}: largest relative deviation of the hyper-step {worst:.3g}, {clamps} clamps")
    assert worst <= HYPER_TOL and clamps > 0


def test_sweep_of_the_double_equals_the_reference(la):
    """one sweep of lr_run_hs over pr.CPU_CASES in float64: beta within pr.F64_TOL, the Polya-Gamma counters equal, the hyper-state within
    1e-12 of the reference's hyper-step at the double's own new beta"""
    worst_b = worst_h = 0.0
    for case in pr.CPU_CASES:
        X, y, ps, st = pr.make_case(case)
        mask, tau0, hyper = hr.case_prior(case)
        ch = np.arange(case.C) + case.chain_offset
        ref = hr.sweep(pr.signed_rows(X, y), ps, st, hyper, mask, tau0, case.seed, ch, case.iter_offset)
        new, h, cn = hr.library_sweep(la, case, "float64", mask, tau0, hyper)
        assert np.array_equal(cn["proposals"], ref.proposals) and np.array_equal(cn["series_terms"], ref.terms) and not cn["skipped"].any() and not ref.skipped.any(), case
        hh, hcn = hr.hyper_step(new, hyper, mask, tau0, case.seed, ch, case.iter_offset)
        assert np.array_equal(cn["clamped"], hcn)
        worst_b, worst_h = max(worst_b, pr.rel_dev(new, ref.beta)), max(worst_h, hr.hyper_dev(h, hh))
    print(f"double vs reference: beta {worst_b:.3g} (F64_TOL {pr.F64_TOL:g}), hyper-state {worst_h:.3g}")
    assert worst_b <= pr.F64_TOL and worst_h <= HYPER_TOL


def test_empty_shrink_set_equals_pg_on_the_double(la):
    from logreg_amd import _lib
    L = _lib.load_hs()
    for dtype in ("float64", "float32"):
        case = pr.CPU_CASES[3]
        X, y, ps, st = pr.make_case(case)
        m = la.LogReg(X, y, ps, dtype=dtype)
        opts = hr._opts(case, iters=3)
        a, b = (np.ascontiguousarray(st, dtype=m.np_dtype).copy() for _ in range(2))
        oa, ob = (np.zeros((3, case.C, case.p), dtype=m.np_dtype) for _ in range(2))
        ca, cb = np.zeros(case.C, dtype=la.kernels.PG_COUNTERS), np.zeros(case.C, dtype=la.kernels.HS_COUNTERS)
        keep, prior = hr._prior(np.zeros(case.p, bool), 1.0)
        h = hr.default_hyper(case.C, case.p, 1.0)
        assert L.lr_run_pg(m.handle, a.ctypes.data, ctypes.byref(opts), oa.ctypes.data, ca.ctypes.data) == 0
        assert L.lr_run_hs(m.handle, ctypes.byref(prior), b.ctypes.data, h.ctypes.data, ctypes.byref(opts), ob.ctypes.data, None, cb.ctypes.data) == 0, L.lr_last_error()
        assert a.tobytes() == b.tobytes() and oa.tobytes() == ob.tobytes()
        assert all(np.array_equal(ca[f], cb[f]) for f in ("proposals", "series_terms", "skipped"))
        assert np.array_equal(h[:, :2 * case.p], np.ones((case.C, 2 * case.p))) and not np.array_equal(h[:, 2 * case.p], np.ones(case.C))  # tau^2 moves under its prior
        m.close()


def test_python_face_on_the_double(la, pima, pscale, map_beta, tmp_path):
    X, y = pima
    with pytest.raises(TypeError, match="X, y"):
        la.hsKernel(lambda b: -0.5 * np.sum(b * b))
    for dtype in ("float64", "float32"):
        m = la.LogReg(X, y, pscale, dtype=dtype)
        # every refusal of the constructor
        with pytest.raises(TypeError, match="not from a log-density"):
            la.hsKernel(m.glp)
        for bad in (np.ones(7, bool), np.ones(8), np.ones((8, 1), bool), [1] * 8):
            with pytest.raises(ValueError, match="boolean mask"):
                la.hsKernel(m.lpost, shrink=bad)
        with pytest.raises(ValueError, match="no coordinate"):
            la.hsKernel(m.lpost, shrink=np.zeros(8, bool))
        for bad in (0, -1.0, np.inf, np.nan, "x", None):
            with pytest.raises(ValueError, match="global_scale"):
                la.hsKernel(m.lpost, global_scale=bad)
        # default mask and start
        k = la.hsKernel(m.lpost)
        assert isinstance(k, la.FusedKernel) and k.kind == "hs" and k.model is m and sorted(k.params) == ["global_scale", "shrink"]
        assert np.array_equal(k.params["shrink"], np.arange(8) > 0) and k.params["global_scale"] == 1.0
        k = la.hsKernel(m.lpost, global_scale=0.25)
        rng = np.random.default_rng(3)
        q0 = map_beta + 0.05 * rng.standard_normal((9, 8))
        cs = la.ChainSet(k, q0, seed=17, chain_offset=2)
        h0 = cs.get_hyper()
        assert h0.shape == (9, 18) and np.array_equal(h0[:, :16], np.ones((9, 16))) and np.array_equal(h0[:, 16], np.full(9, 0.0625)) and np.array_equal(h0[:, 17], np.ones(9))
        assert cs.plan()["group"] >= 1
        for bad in (np.zeros(18), np.full(18, np.nan), np.full(18, 1e101), np.full((9, 18), -1.0)):
            with pytest.raises(ValueError, match="hyper-state"):
                cs.set_hyper(bad)
        with pytest.raises(ValueError, match="horseshoe"):
            la.ChainSet(la.pgKernel(m.lpost), q0, seed=1).get_hyper()
        with pytest.raises(ValueError, match="horseshoe"):
            la.ChainSet(la.pgKernel(m.lpost), q0, seed=1).advance(2, 1, scales=la.DeviceArray(m.device, (2, 9, 9), np.float64))
        with pytest.raises(ValueError, match="p\\+1"):
            cs.advance(2, 1, scales=la.DeviceArray(m.device, (2, 9, 8), np.float64))
        # the bridge refusal, with the reason
        with pytest.raises(ValueError, match="Gaussian prior"):
            la.mcmc(q0, k, thin=1, iters=2, verb=False, seed=1, bridge=object())
        # a run and its info
        full, info = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, return_info=True)
        assert full.shape == (6, 9, 8) and full.dtype == m.np_dtype and np.all(np.isfinite(full))
        assert {"state", "seed", "plan", "iterations", "proposals", "series_terms", "skipped", "clamped", "proposals_per_draw", "series_terms_per_draw", "hyper",
                "local_scale2", "global_scale2"} <= set(info)
        assert info["local_scale2"].shape == (6, 9, 8) and info["global_scale2"].shape == (6, 9) and info["hyper"].shape == (9, 18) and info["iterations"] == 12
        assert np.array_equal(info["local_scale2"][:, :, 0], np.ones((6, 9))) and np.all(info["local_scale2"][:, :, 1:] != 1.0)
        assert np.array_equal(info["local_scale2"][-1], np.where(k.params["shrink"], info["hyper"][:, :8], 1.0)) and np.array_equal(info["global_scale2"][-1], info["hyper"][:, 16])
        assert info["skipped"].sum() == 0 and info["clamped"].sum() == 0 and np.all(info["proposals"] >= m.n * 12)
        if dtype == "float64":  # the whole run against the reference: 12 sweeps compound
            Xs, beta, hyper = pr.signed_rows(X, y), q0.copy(), hr.default_hyper(9, 8, 0.25)
            for it in range(12):
                s = hr.sweep(Xs, pscale, beta, hyper, k.params["shrink"], 0.25, 17, np.arange(9) + 2, it)
                beta, hyper = s.beta, s.hyper
            assert pr.rel_dev(full[-1], beta) <= pr.F64_TOL * 12 and hr.hyper_dev(info["hyper"], hyper) <= 1e-9
        # chunks, shards, the single-chain form, one step
        parts, pinfo = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, chunk=4, return_info=True)
        assert np.array_equal(parts, full) and all(np.array_equal(pinfo[f], info[f]) for f in ("hyper", "local_scale2", "global_scale2", "clamped", "proposals"))
        sh, shi = la.mcmc(q0[3:8], k, thin=2, iters=6, verb=False, seed=17, chain_offset=5, plan_chains=9, plan_first=2, return_info=True)
        assert np.array_equal(sh, full[:, 3:8]) and np.array_equal(shi["hyper"], info["hyper"][3:8]) and np.array_equal(shi["local_scale2"], info["local_scale2"][:, 3:8])
        one, oinfo = la.mcmc(map_beta, k, thin=1, iters=3, verb=False, seed=5, return_info=True)
        assert one.shape == (3, 8) and one.dtype == np.float64 and oinfo["local_scale2"].shape == (3, 8) and oinfo["global_scale2"].shape == (3,)
        x1 = k(map_beta)
        x2 = k(x1)
        assert x1.shape == (8,) and np.all(np.isfinite(x2)) and not np.array_equal(x1, x2) and not np.array_equal(k._hyper, hr.default_hyper(1, 8, 0.25))
        # checkpoint: the hyper-state and the counters travel
        cs = la.ChainSet(k, q0, seed=17, chain_offset=2)
        a = cs.advance(2, 2).to_host()
        cs2 = la.ChainSet.resume(k, cs.save(tmp_path / f"hs_{dtype}"))
        assert np.array_equal(cs2.get_hyper(), cs.get_hyper()) and not np.array_equal(cs2.get_hyper(), h0)
        b = cs2.advance(4, 2).to_host()
        assert np.array_equal(np.concatenate([a, b]), full) and np.array_equal(cs2.get_hyper(), info["hyper"])
        for f in ("proposals", "series_terms", "skipped", "clamped"):
            assert np.array_equal(cs2.get_counters()[f], info[f]), f
        with pytest.raises(ValueError, match="param_shrink"):
            la.ChainSet.resume(la.hsKernel(m.lpost, shrink=np.arange(8) > 1, global_scale=0.25), cs.checkpoint())
        with pytest.raises(ValueError, match="checkpoint is for"):
            la.ChainSet.resume(la.pgKernel(m.lpost), cs.checkpoint())
        # set_hyper moves the run
        cs3 = la.ChainSet(k, q0, seed=17, chain_offset=2)
        cs3.set_hyper(np.full(18, 1e-3))
        assert np.array_equal(cs3.get_hyper(), np.full((9, 18), 1e-3)) and not np.array_equal(cs3.advance(2, 2).to_host(), a)
        # a non-finite start stays in place, hyper-state included, and is counted
        bad = q0.copy()
        bad[1, 3], bad[4, 0] = np.nan, np.inf
        out, binfo = la.mcmc(bad, k, thin=2, iters=3, verb=False, seed=17, return_info=True)
        for c in (1, 4):
            assert binfo["skipped"][c] == 6 and binfo["proposals"][c] == 0 and binfo["clamped"][c] == 0 and np.array_equal(binfo["hyper"][c], h0[c])
            assert np.array_equal(binfo["local_scale2"][:, c], np.ones((3, 8))) and np.array_equal(binfo["global_scale2"][:, c], np.full(3, 0.0625))
        # summary_only: the streaming statistics of the same run, the final hyper-state and the counters
        res = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, summary_only=True)
        assert res["accept_rate"] == 1.0 and np.array_equal(res["proposals"], info["proposals"]) and np.array_equal(res["hyper"], info["hyper"]) and "clamped" in res
        np.testing.assert_allclose(res["mean"], full.astype(np.float64).mean(axis=(0, 1)), rtol=1e-6)
        m.close()


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_hs.h") == WANT == sorted(_lib.HS_SYMBOLS)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PG_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.ADAPT_SYMBOLS,
                  _lib.DENSE_SYMBOLS, _lib.BRIDGE_SYMBOLS, _lib.RANK_SYMBOLS, _lib.PPC_SYMBOLS):
        assert not set(WANT) & set(other)
    L = ctypes.CDLL(twin_hs.build())
    for s in WANT + _declared("logreg_hip_pg.h") + _declared("logreg_hip.h"):
        assert hasattr(L, s)
    assert _lib.HS_TAG == 0x02000000 and ctypes.sizeof(_lib.HsCounters) == 24 and ctypes.sizeof(_lib.HsPrior) == 16
    import logreg_amd.kernels as K
    assert K.HS_COUNTERS.itemsize == 24 and K.HS_COUNTERS.names == tuple(f for f, _ in _lib.HsCounters._fields_)
    txt = open(os.path.join(REPO, "include", "logreg_hip_hs.h")).read()
    for word in ("#define LR_HS_TAG 0x02000000u", "#define LR_HS_MIN 1e-100", "#define LR_HS_MAX 1e100", "ACCEPT m = 0", "Order of the sum", "depends on (seed, chain, iteration"):
        assert word in txt, word
    assert "0x02000000" in open(os.path.join(build.CSRC, "lr_device.h")).read()
    src = build._sources()
    for f in (os.path.join(build.INCLUDE, "logreg_hip_hs.h"), os.path.join(build.CSRC, "lr_hs.h")):
        assert f in src, f
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_run_hs|lr_hs_\w+)\b", exported))) == WANT, path


def test_the_eight_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        rows = [r for r in b.kernel_resources(alt=alt) if "k_hs<" in r["name"]]
        assert len(rows) == 8 and len(b.unit_objects(alt)) == 13 and not any("k_pg<" in r["name"] for r in rows)
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32):
                mine = [r for r in rows if f"k_hs<{dt}, {P}>" in r["name"]]
                assert len(mine) == 1 and mine[0]["unit"] == f"lr_inst_{'f32' if dt == 'float' else 'f64'}_p{P}", (alt, dt, P)
        assert all(r["scratch"] == 0 and r["lds"] == 0 and r["vgprs"] + r["agprs"] <= 512 for r in rows), [(r["name"], r["scratch"], r["vgprs"], r["agprs"]) for r in rows]
        assert isa_gate.scan_paths(b.unit_objects(alt)) == []


def test_host_side_under_asan_and_ubsan():
    """tests/host/hs_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's instantiation
    objects by tests/host_build.py: every refusal ahead of any device access, runs from host and device memory on the stub, every
    allocation failing in turn."""
    last = host_build.last_line(host_build.run(host_build.harness("hs_harness.cpp")))
    assert last.startswith("hs harness:"), last
