"""Posterior covariance and correlation on the device (include/logreg_hip_cov.h, logreg_amd/covariance.py) -- everything that can be
checked without a GPU: the ABI tables, the build gates with the new kernels in both builds, result_from_tables on the reference's tables
against np.cov, np.corrcoef and a direct NumPy W / B / lambda_max within the propagated bounds, the NumPy merge, the metric conventions,
argument validation ahead of any device access, and the host side of the accumulator (tests/host/cov_harness.cpp, a stand-alone
program) under AddressSanitizer and UBSan."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import host_build
import cov_cases as cases
import cov_reference as cr

WANT = ["lr_cov_accumulate", "lr_cov_create", "lr_cov_destroy", "lr_cov_reset", "lr_cov_result"]
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = cases.case(name, dtype)
        _REF[(name, dtype)] = cr.tables(c["x"], c["center"], c["scale"])
    return _REF[(name, dtype)]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_cov.h") == WANT == sorted(_lib.COV_SYMBOLS)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS):
        assert not set(WANT) & set(other)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_cov_\w+)", exported))) == WANT, path
    hdr = open(os.path.join(REPO, "include", "logreg_hip_cov.h")).read()
    assert _lib.COV_MAX_P == int(re.search(r"#define LR_COV_MAX_P (\d+)", hdr).group(1)) == 128
    assert _lib.load_covariance() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_cov.h") in src and os.path.join(build.CSRC, "lr_cov.h") in src


def test_still_13_units_and_the_covariance_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_cov_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32, 64, 128):
                assert sum(f"k_cov_accumulate<{dt}, {P}>" in r["name"] for r in mine) == 1, (alt, dt, P)
        for k in ("k_cov_init", "k_cov_runs", "k_cov_outer"):
            assert sum(k in r["name"] for r in mine) == 1, (alt, k)
        assert len(mine) == 15
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert all(r["lds"] <= 32 * 1024 for r in mine)
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_tables_are_non_finite_exactly_where_a_draw_is(name):
    for dtype in cases.DTYPES:
        c = cases.case(name, dtype)
        ref = reference(name, dtype)
        p = c["p"]
        assert ref["moment"].shape == (p, p) and ref["chain_sums"].shape == (c["C"], p)
        if name.endswith("_same"):
            N = c["n"] * c["C"]
            assert np.all(ref["moment"] == 0.25 * N) and np.all(ref["sum"] == 0.5 * N) and np.all(ref["chain_sums"] == 0.5 * c["n"])
        elif c["C"] >= 5:
            assert not ref["finite"][0] and not ref["finite"][p - 1] and ref["finite"].sum() == max(0, p - 2)
            assert not np.isfinite(ref["chain_sums"][3, 0]) and not np.isfinite(ref["chain_sums"][4, p - 1])
            assert np.isfinite(ref["chain_sums"]).sum() == c["C"] * p - (2 if p > 1 else 2)
            if p >= 3:
                assert np.isfinite(ref["moment"]).sum() == (p - 2) ** 2 == np.isfinite(ref["chain_outer"]).sum()
        else:
            assert ref["finite"].all() and all(np.isfinite(ref[k]).all() for k in ("moment", "chain_outer", "sum", "chain_sums"))
        # the bounds are tight enough to tell a wrong kernel: a relative 1e-9 of the scale of the entry
        ok = np.isfinite(ref["moment"])
        T = ref["tol_moment"][ok] / ((c["n"] * c["C"] + 8) * cr.EPS)
        assert np.all(ref["tol_moment"][ok] <= 1e-9 * T)


@pytest.mark.parametrize("name", cases.NAMES)
def test_result_from_tables_on_the_reference_tables_is_numpys_cov_corrcoef_w_b_and_lambda_max(name):
    from logreg_amd.covariance import result_from_tables
    seen = 0
    for dtype in cases.DTYPES:
        c = cases.case(name, dtype)
        ref = reference(name, dtype)
        J = np.flatnonzero(ref["finite"])
        if J.size == 0:
            continue
        ix = np.ix_(J, J)
        n, C = c["n"], c["C"]
        res = result_from_tables(ref["moment"][ix], ref["chain_outer"][ix], ref["sum"][J], ref["chain_sums"][:, J], n, c["center"][J], c["scale"][J])
        assert res["nobs"] == n * C and res["chains"] == C and res["n_draws"] == n
        want = cr.derived(c["x"][:, :, J])
        tol = cr.derived_bounds(ref, J, c["center"], c["scale"])
        if name.endswith("_same"):
            assert np.all(res["cov"] == 0) and np.all(np.isnan(res["cor"])) and np.all(res["sd"] == 0) and np.all(res["mean"] == 1.25)
            assert np.isnan(res["rhat_mv"])
            continue
        for key in ("mean", "cov", "cor") + (("within",) if n > 1 else ()) + (("between",) if C > 1 else ()):
            if key == "cor" and n * C < 2:
                continue
            err, t = np.abs(res[key] - want[key]), 2.0 * tol["tol_" + key]
            assert np.all(np.isfinite(t)) and np.all(err <= t), (name, dtype, key, float(np.max(err / t)))
            seen += 1
        assert np.array_equal(res["sd"], np.sqrt(np.diag(res["cov"]))) and np.all(np.diag(res["cor"]) == 1.0)
        assert np.all(np.abs(res["cor"]) <= 1.0 + 1e-12)
        if np.isfinite(want["lam"]) and np.isfinite(tol["tol_lam"]):
            assert abs(res["rhat_mv"] - want["rhat_mv"]) <= (C + 1) / C * 2.0 * tol["tol_lam"], (name, dtype, res["rhat_mv"], want["rhat_mv"], tol["tol_lam"])
            assert np.allclose(res["rhat"], want["rhat"], rtol=1e-9, atol=0)
            assert np.allclose(res["mcse_chains"], np.sqrt(np.diag(want["between"]) / (n * C)), rtol=1e-6)
            seen += 1
        else:
            assert np.isnan(res["rhat_mv"]), (name, dtype, res["rhat_mv"])  # C < 2, n < 2 or a singular W
    assert seen or name in ("C300_p1_n40", "C37_p8_n64_same")


def test_the_multivariate_rhat_is_checked_on_some_case_and_correlations_span_the_range():
    lams = []
    for name in cases.NAMES:
        c = cases.case(name, "float64")
        J = np.flatnonzero(reference(name, "float64")["finite"])
        if J.size and not name.endswith("_same"):
            lams.append(cr.derived(c["x"][:, :, J])["lam"])
    assert sum(np.isfinite(v) for v in lams) >= 4
    cor = cr.derived(cases.case("C5_p20_n200", "float64")["x"][:, :, 1:19])["cor"]
    off = cor[~np.eye(18, dtype=bool)]
    assert off.min() < -0.8 and off.max() > 0.8


def test_merge_covariance_of_two_chain_shards_is_the_whole():
    from logreg_amd import merge_covariance
    from logreg_amd.covariance import result_from_tables
    c = cases.case("C37_p8_n64", "float64")
    J = np.arange(1, 7)
    x = c["x"][:, :, J]
    ctr, scl = c["center"][J], c["scale"][J]
    t = lambda r: (r["moment"], r["chain_outer"], r["sum"], r["chain_sums"])  # noqa: E731
    whole = cr.tables(x, ctr, scl)
    parts = [cr.tables(x[:, :20], ctr, scl), cr.tables(x[:, 20:], ctr, scl)]
    want = result_from_tables(*t(whole), 64, ctr, scl)
    res = merge_covariance([result_from_tables(*t(q), 64, ctr, scl) for q in parts])
    raw = merge_covariance([(*t(q), 64) for q in parts], center=ctr, scale=scl)
    for got in (res, raw):
        assert got["chains"] == 37 and got["n_draws"] == 64 and got["nobs"] == 64 * 37
        assert np.array_equal(got["chain_sums"], want["chain_sums"])
        for key in ("moment", "chain_outer", "sum", "mean", "cov", "cor", "within", "between", "rhat", "mcse_chains"):
            assert np.allclose(got[key], want[key], rtol=1e-11, atol=1e-13), key
        assert got["rhat_mv"] == pytest.approx(want["rhat_mv"], rel=1e-9)
    with pytest.raises(ValueError):
        merge_covariance([])
    with pytest.raises(ValueError, match="same center and scale"):
        merge_covariance([want, result_from_tables(*t(whole), 64, ctr + 1.0, scl)])
    with pytest.raises(ValueError, match="same n"):
        merge_covariance([want, result_from_tables(*t(whole), 65, ctr, scl)])
    with pytest.raises(ValueError, match="center= and scale="):
        merge_covariance([(*t(whole), 64)])


def test_metric_conventions_scaling_and_the_empty_result():
    from logreg_amd import covariance_scaling
    from logreg_amd.covariance import metric, result_from_tables
    rng = np.random.default_rng(3)
    x = rng.standard_normal((50, 4, 3)) * np.array([0.1, 2.0, 30.0]) + np.array([5.0, -1.0, 0.0])
    ctr, scl = covariance_scaling([5.0, -1.0, 0.0], [0.1, 2.0, 30.0])
    assert np.array_equal(ctr, [5.0, -1.0, 0.0]) and np.array_equal(scl, 1.0 / np.array([0.1, 2.0, 30.0])) and scl.dtype == np.float64
    r = cr.tables(x, ctr, scl)
    res = result_from_tables(r["moment"], r["chain_outer"], r["sum"], r["chain_sums"], 50, ctr, scl)
    m = metric(res)
    var = np.var(x.reshape(-1, 3), axis=0, ddof=1)
    assert set(m) == {"dmm", "pre"} and np.allclose(m["pre"], var, rtol=1e-12) and np.allclose(m["dmm"], 1.0 / var, rtol=1e-12)
    assert np.array_equal(m["dmm"] * m["pre"], np.ones(3)) or np.allclose(m["dmm"] * m["pre"], 1.0, rtol=1e-15)
    for bad in (([1.0], [0.0]), ([1.0], [-1.0]), ([np.nan], [1.0]), ([1.0, 2.0], [1.0]), (1.0, 1.0), ([1.0], [np.inf]), ([1.0], [1e-320])):
        with pytest.raises(ValueError):
            covariance_scaling(*bad)
    nan = np.full((3, 3), np.nan)
    empty = result_from_tables(nan, nan, np.full(3, np.nan), np.full((4, 3), np.nan), 0, ctr, scl)  # what an accumulator holds before the first draw
    assert empty["nobs"] == 0 and np.all(np.isnan(empty["cov"])) and np.all(np.isnan(empty["mean"])) and np.isnan(empty["rhat_mv"])
    with pytest.raises(ValueError, match="positive variance"):
        metric(empty)
    one = result_from_tables(r["moment"], r["chain_outer"], r["sum"], r["chain_sums"][:1] * 4, 200, ctr, scl)  # one chain: no B, no R-hat
    assert np.all(np.isnan(one["between"])) and np.isnan(one["rhat_mv"]) and np.all(np.isfinite(one["cov"]))
    with pytest.raises(ValueError):
        result_from_tables(r["moment"], r["chain_outer"][:2], r["sum"], r["chain_sums"], 50, ctr, scl)


def test_covariance_validates_before_any_device_access(pima, pscale):
    import logreg_amd as la
    good = dict(chains=5, p=3, dtype="float32", center=[0.0, 0.0, 0.0], scale=[1.0, 2.0, 3.0])
    for bad in (dict(dtype="float16"), dict(dtype="int32"), dict(chains=0), dict(p=0), dict(p=129, center=np.zeros(129), scale=np.ones(129)),
                dict(scale=[1.0, 0.0, 1.0]), dict(scale=[1.0, -2.0, 1.0]), dict(scale=[1.0, np.inf, 1.0]), dict(scale=[1.0, np.nan, 1.0]),
                dict(center=[0.0, np.nan, 0.0]), dict(center=[-np.inf, 0.0, 0.0]), dict(center=[0.0, 0.0]), dict(scale=[1.0, 2.0, 3.0, 4.0]),
                dict(center=None), dict(scale=None)):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            la.Covariance(**kw)
    acc = la.Covariance(5, 3, "float64", [0.0, 0.0, 0.0], [1.0, 2.0, 3.0])  # no device yet: nothing is allocated before the first block
    assert acc.n_draws == 0 and acc.dtype == np.float64 and acc._h is None and "Covariance(chains=5, p=3" in repr(acc)
    for block in (np.zeros((4, 5)), np.zeros((4, 3, 5)), np.zeros((4, 5, 4)), np.zeros((0, 5, 3)), np.zeros((4, 5, 3), dtype=complex)):
        with pytest.raises(ValueError):
            acc.update(block)
    assert acc._h is None and acc.n_draws == 0
    if la.device_count() == 0:
        with pytest.raises(la.LogregHipError, match="no CPU fallback"):
            acc.update(np.zeros((4, 5, 3)))
    # mcmc(covariance=): keyword-only, ahead of marginals and predictive (which stay last), refused with a reason before anything runs
    params = inspect.signature(la.mcmc).parameters
    par = params["covariance"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert list(params)[-3:] == ["covariance", "marginals", "predictive"]
    with pytest.raises(ValueError, match="needs a fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, covariance=la.Covariance(1, 2, center=[0, 0], scale=[1, 1]))
    import twin
    from logreg_amd import _lib
    X, y = pima
    L = twin.install()
    try:
        assert _lib.load() is L and not hasattr(L, "lr_cov_create")
        model = la.LogReg(X, y, pscale, dtype="float64")
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.zeros((6, 8))
        c8, s8 = np.zeros(8), np.ones(8)
        for wrong in (la.Covariance(5, 8, "float64", c8, s8), la.Covariance(6, 7, "float64", c8[:7], s8[:7]), la.Covariance(6, 8, "float32", c8, s8),
                      la.Covariance(6, 8, "float64", c8, s8, device=1)):
            with pytest.raises(ValueError, match="covariance= is for"):
                la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, covariance=wrong)
        with pytest.raises(ValueError, match="must be a Covariance"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, covariance="yes")
        with pytest.raises(ValueError, match="must be a Covariance"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, covariance=la.Marginals(6, 8, "float64", -s8, s8))
        with pytest.raises(la.LogregHipError, match="no covariance entry points"):  # a library without the new header says so
            la.Covariance(6, 8, "float64", c8, s8).update(np.zeros((2, 6, 8)))
        model.close()
    finally:
        twin.uninstall()


def test_host_side_of_the_accumulator_under_asan_and_ubsan():
    """tests/host/cov_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's instantiation
    objects by tests/host_build.py: both dtypes, a padded and an unpadded p, host and device
    input, every refused argument, a failing allocation at every allocation of create, accumulate and result."""
    last = host_build.last_line(host_build.run(host_build.harness("cov_harness.cpp")))
    assert last.startswith("cov harness:"), last
    assert int(last.split(":")[1].split("kernel launches")[0]) > 100, last
