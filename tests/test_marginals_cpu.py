"""Marginal histograms, quantiles and moments on the device (include/logreg_hip_marginals.h, logreg_amd/marginals.py) -- everything that can
be checked without a GPU: the ABI tables, the build gates with the new kernels in both builds, the independent reference against scipy,
the condition on its bounds, the quantile guarantee, interval / hpd, the NumPy merge, and argument validation ahead of any device access."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import marginals_cases as cases
import marginals_reference as mr

WANT = ["lr_marg_accumulate", "lr_marg_create", "lr_marg_destroy", "lr_marg_reset", "lr_marg_result"]
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = cases.case(name, dtype)
        _REF[(name, dtype)] = mr.reference(c["x"], c["lo"], c["hi"], c["B"])
    return _REF[(name, dtype)]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_marginals.h") == WANT == sorted(_lib.MARG_SYMBOLS)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_marg_\w+)", exported))) == WANT, path
    hdr = open(os.path.join(REPO, "include", "logreg_hip_marginals.h")).read()
    assert _lib.MARG_MAX_BINS == int(re.search(r"#define LR_MARG_MAX_BINS (\d+)", hdr).group(1)) == 1024
    assert _lib.MARG_ROWS == int(re.search(r"#define LR_MARG_ROWS (\d+)", hdr).group(1)) == 6
    assert re.search(r"#define LR_MARG_COLS\(B\) \(\(B\) \+ (\d+)\)", hdr).group(1) == "3"
    assert _lib.load_marginals() is _lib.load()  # binds on first use


def test_the_older_symbol_sets_are_unchanged():
    from logreg_amd import _lib
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    assert _declared("logreg_hip_nuts.h") == sorted(_lib.NUTS_SYMBOLS) == ["lr_run_nuts"]
    assert _declared("logreg_hip_predict.h") == sorted(_lib.PREDICT_SYMBOLS) == [
        "lr_predict_accumulate", "lr_predict_create", "lr_predict_destroy", "lr_predict_reset", "lr_predict_result"]
    assert _declared("logreg_hip_acf.h") == sorted(_lib.ACF_SYMBOLS) == [
        "lr_acf_accumulate", "lr_acf_create", "lr_acf_destroy", "lr_acf_reset", "lr_acf_result"]
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS):
        assert not set(WANT) & set(other)


def test_header_and_kernels_are_part_of_the_build_id():
    from logreg_amd import build
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_marginals.h") in src and os.path.join(build.CSRC, "lr_marginals.h") in src


def test_still_13_units_and_the_marginals_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_marg_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):
            assert sum(f"k_marg_accumulate<{dt}>" in r["name"] for r in mine) == 1, (alt, dt)
        for k in ("k_marg_init", "k_marg_partial", "k_marg_final"):
            assert sum(k in r["name"] for r in mine) == 1, (alt, k)
        assert len(mine) == 5
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)  # (the second build may use scratch in older kernels: its gate only reports)


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_counts_sum_to_the_number_of_draws_and_the_special_series_are_where_they_belong(name):
    for dtype in cases.DTYPES:
        c = cases.case(name, dtype)
        ref = reference(name, dtype)
        B, p = c["B"], c["p"]
        assert ref["counts"].shape == (p, B + 3) and np.all(ref["counts"].sum(axis=1) == c["n"] * c["C"])
        if name.endswith("_same"):
            assert np.all(ref["counts"][:, 1 + (5 * B) // 8] == c["n"] * c["C"])  # 1.25 on [0, 2): every draw in one bin
            assert np.all(ref["table"][:2] == 1.25) and np.all(ref["variance"] == 0) and not ref["shaped"].any()
        elif c["C"] >= 5:
            jf = 1 if p >= 3 else 0
            x = c["x"]
            assert x[0, 2, jf] == c["lo"][jf] and x[1, 2, jf] == c["hi"][jf] and x[2, 2, jf] < c["hi"][jf]
            assert x[2, 2, jf] == np.nextafter(np.asarray(c["hi"][jf], dtype=dtype), np.asarray(-np.inf, dtype=dtype))
            col = mr.columns(x[:5, 2, jf], c["lo"][jf], c["hi"][jf], B)
            assert col[0] == 1 and col[1] == B + 1 and col[2] in (B, B + 1) and col[3] == 0 and col[4] == B + 1
            assert ref["counts"][jf, 0] >= 1 and ref["counts"][jf, B + 1] >= 2 and ref["counts"][0, B + 2] == 1
            assert ref["table"][0, p - 1] == -np.inf and ref["table"][1, p - 1] == np.inf
            assert not ref["finite"][0] and not ref["finite"][p - 1] and not np.isfinite(ref["table"][2:, [0, p - 1]]).any()
            assert p == 1 or np.isfinite(ref["table"][:2, 0]).all()  # min / max skip the NaN
            if p >= 3:
                assert ref["finite"][jf] and ref["shaped"][jf] and np.isfinite(ref["table"][:, jf]).all()


def test_reference_moments_are_scipys_describe():
    st = pytest.importorskip("scipy.stats")
    seen = 0
    for name in cases.NAMES:
        for dtype in cases.DTYPES:
            c = cases.case(name, dtype)
            ref = reference(name, dtype)
            ok = ref["shaped"]
            if not ok.any():
                continue
            d = st.describe(c["x"].reshape(-1, c["p"])[:, ok], axis=0)
            assert d.nobs == c["n"] * c["C"]
            for got, want in ((ref["table"][0, ok], d.minmax[0]), (ref["table"][1, ok], d.minmax[1]), (ref["mean"][ok], d.mean),
                              (ref["variance"][ok], d.variance), (ref["skewness"][ok], d.skewness), (ref["kurtosis"][ok], d.kurtosis)):
                assert np.allclose(got, want, rtol=1e-10, atol=1e-10), (name, dtype)
            seen += int(ok.sum())
    assert seen > 250


@pytest.mark.parametrize("name", cases.NAMES)
def test_bounds_are_tight_enough_to_tell_a_wrong_kernel(name):
    """Every case's bound on skewness and on kurtosis is <= 1e-8: a loose bound must not be able to hide a wrong kernel."""
    for dtype in cases.DTYPES:
        ref = reference(name, dtype)
        ok = ref["shaped"]
        if ok.any():
            assert np.all(ref["tol_skewness"][ok] <= 1e-8) and np.all(ref["tol_kurtosis"][ok] <= 1e-8), (
                name, dtype, ref["tol_skewness"][ok].max(), ref["tol_kurtosis"][ok].max())


def test_some_coordinate_of_every_shape_is_checked_for_shape():
    got = {name: int(reference(name, "float64")["shaped"].sum()) for name in cases.NAMES}
    assert got["C37_p8_n64_B64"] == 6 and got["C5_p20_n200_B256"] == 18 and got["C130_p3_n601_B1024"] == 1
    assert got["C1_p1_n7_B8"] == 1 and got["C3_p128_n16_B1024"] == 128


@pytest.mark.parametrize("name", cases.NAMES)
def test_quantile_lies_in_the_column_of_the_order_statistic(name):
    from logreg_amd.marginals import quantile, result_from_tables
    for dtype in cases.DTYPES:
        c = cases.case(name, dtype)
        ref = reference(name, dtype)
        res = result_from_tables(ref["counts"], ref["table"], c["lo"], c["hi"], c["n"], c["C"])
        q = quantile(res, cases.QS)
        assert q.shape == (len(cases.QS), c["p"]) and np.array_equal(quantile(res, 0.5), q[4])
        X = c["x"].reshape(-1, c["p"])
        for j in range(c["p"]):
            if not ref["finite"][j]:
                continue
            exact = np.quantile(X[:, j], cases.QS, method="inverted_cdf")
            want = mr.columns(exact, c["lo"][j], c["hi"][j], c["B"])
            got = mr.columns(q[:, j], c["lo"][j], c["hi"][j], c["B"])
            assert np.array_equal(got, want), (name, dtype, j, q[:, j], exact)
            assert np.all(q[:, j] >= ref["table"][0, j]) and np.all(q[:, j] <= ref["table"][1, j]) and np.all(np.diff(q[:, j]) >= 0)
            inside = (want >= 1) & (want <= c["B"])
            assert np.all(np.abs(q[:, j] - exact)[inside] <= (c["hi"][j] - c["lo"][j]) / c["B"] * (1 + 1e-12))


def _hand_made():
    from logreg_amd.marginals import result_from_tables
    # one coordinate, 4 bins on [0, 4): columns = underflow, 4 bins, overflow, NaN
    counts = np.array([[2, 10, 60, 20, 6, 2, 5]], dtype=np.uint64)
    table = np.array([[-1.0], [6.0], [0.0], [1.0], [0.0], [1.0]])
    return result_from_tables(counts, table, [0.0], [4.0], 105, 1)


def test_interval_and_hpd_on_a_hand_made_table():
    from logreg_amd.marginals import hpd, interval, quantile
    res = _hand_made()
    assert res["nobs"] == 105 and res["nan"][0] == 5 and res["underflow"][0] == 2 and res["overflow"][0] == 2
    assert np.array_equal(res["counts"], [[10, 60, 20, 6]]) and np.array_equal(res["edges"], [[0, 1, 2, 3, 4]])
    assert np.allclose(res["density"], [[0.10, 0.60, 0.20, 0.06]]) and res["minmax"][0][0] == -1 and res["minmax"][1][0] == 6
    # 100 non-NaN draws: rank 50 is the 38th of the 60 draws of bin [1, 2): 1 + 37.5 / 60
    assert quantile(res, 0.5)[0] == pytest.approx(1 + 37.5 / 60)
    assert quantile(res, 0.0)[0] == pytest.approx(-1 + 0.5 / 2) and quantile(res, 1.0)[0] == pytest.approx(4 + 2 * 1.5 / 2)
    iv = interval(res, 0.9)  # ranks 5 and 95: the 3rd of bin [0, 1), the 3rd of bin [3, 4)
    assert iv.shape == (2, 1) and iv[0, 0] == pytest.approx(2.5 / 10) and iv[1, 0] == pytest.approx(3 + 2.5 / 6)
    assert np.array_equal(hpd(res, 0.6), [[1.0], [2.0]])      # 60 draws: the one bin [1, 2)
    assert np.array_equal(hpd(res, 0.8), [[1.0], [3.0]])      # 80: [1, 3)
    assert np.array_equal(hpd(res, 0.9), [[0.0], [3.0]])      # 90: [0, 3)
    assert np.array_equal(hpd(res, 0.99), [[-1.0], [6.0]])    # 99 of 100: no side can be dropped (2 + 2 outside the grid)
    for bad in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError):
            hpd(res, bad)
        with pytest.raises(ValueError):
            interval(res, bad)
    with pytest.raises(ValueError):
        quantile(res, 1.5)


def test_merge_marginals_of_two_halves_is_the_whole():
    from logreg_amd import merge_marginals
    from logreg_amd.marginals import result_from_tables
    c = cases.case("C37_p8_n64_B64", "float64")
    x = c["x"]
    lo, hi, B = c["lo"], c["hi"], c["B"]
    whole = mr.reference(x, lo, hi, B)
    parts = [mr.reference(x[:, :20], lo, hi, B), mr.reference(x[:, 20:], lo, hi, B)]
    res = merge_marginals([result_from_tables(q["counts"], q["table"], lo, hi, 64, q["C"]) for q in parts])
    want = result_from_tables(whole["counts"], whole["table"], lo, hi, 64, 37)
    assert res["chains"] == 37 and res["n"] == 64 and res["nobs"] == 64 * 37 and res["bins"] == B
    for key in ("columns", "counts", "underflow", "overflow", "nan", "edges"):
        assert np.array_equal(res[key], want[key]), key
    assert np.array_equal(res["minmax"][0], want["minmax"][0]) and np.array_equal(res["minmax"][1], want["minmax"][1])
    ok = whole["finite"]
    assert ok.sum() == 6 and not np.isfinite(res["table"][2:, ~ok]).any()
    for key in ("mean", "variance", "skewness", "kurtosis"):
        assert np.allclose(res[key][ok], want[key][ok], rtol=1e-12, atol=1e-12), key
    assert np.allclose(res["table"][2:, ok], want["table"][2:, ok], rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        merge_marginals([])
    with pytest.raises(ValueError, match="same grid"):
        merge_marginals([want, result_from_tables(whole["counts"], whole["table"], lo, hi + 1.0, 64, 37)])
    with pytest.raises(ValueError, match="same n"):
        merge_marginals([want, result_from_tables(whole["counts"], whole["table"], lo, hi, 65, 37)])


def test_the_library_moments_formula_meets_the_reference_bounds_on_exact_sums():
    """result_from_tables on the reference's own tables: the conversion from power sums to moments alone stays within the bounds."""
    from logreg_amd.marginals import result_from_tables
    for name in cases.NAMES:
        for dtype in cases.DTYPES:
            c = cases.case(name, dtype)
            ref = reference(name, dtype)
            res = result_from_tables(ref["counts"], ref["table"], c["lo"], c["hi"], c["n"], c["C"])
            ratio, bad = mr.compare(ref["counts"], ref["table"], res, ref)
            assert not bad and ratio <= 1.0, (name, dtype, ratio, bad)


def test_marginal_grid():
    from logreg_amd import marginal_grid
    lo, hi = marginal_grid([1.0, -2.0], [0.5, 0.25])
    assert np.array_equal(lo, [-3.0, -4.0]) and np.array_equal(hi, [5.0, 0.0])
    lo, hi = marginal_grid([1.0], [0.5], width=2.0)
    assert lo[0] == 0.0 and hi[0] == 2.0
    for bad in (([1.0], [0.0]), ([1.0], [-1.0]), ([np.nan], [1.0]), ([1.0, 2.0], [1.0]), (1.0, 1.0)):
        with pytest.raises(ValueError):
            marginal_grid(*bad)
    with pytest.raises(ValueError):
        marginal_grid([1.0], [1.0], width=0.0)


def test_marginals_validates_before_any_device_access(pima, pscale):
    import logreg_amd as la
    good = dict(chains=5, p=3, dtype="float32", lo=[0.0, 0.0, 0.0], hi=[1.0, 2.0, 3.0])
    for bad in (dict(bins=0), dict(bins=1025), dict(bins=-3), dict(dtype="float16"), dict(dtype="int32"), dict(chains=0), dict(p=0),
                dict(lo=[0.0, 2.0, 0.0]), dict(lo=[0.0, 3.0, 0.0]), dict(lo=[0.0, np.nan, 0.0]), dict(lo=[-np.inf, 0.0, 0.0]),
                dict(hi=[1.0, np.inf, 3.0]), dict(lo=[0.0, 0.0]), dict(hi=[1.0, 2.0, 3.0, 4.0]), dict(lo=None), dict(hi=None),
                dict(lo=[-1e308, 0.0, 0.0], hi=[1e308, 1.0, 1.0])):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            la.Marginals(**kw)
    mg = la.Marginals(5, 3, "float64", [0.0, 0.0, 0.0], [1.0, 2.0, 3.0])  # no device yet: nothing is allocated before the first block
    assert mg.bins == 256 and mg.n_draws == 0 and mg.dtype == np.float64 and mg._h is None
    for block in (np.zeros((4, 5)), np.zeros((4, 3, 5)), np.zeros((4, 5, 4)), np.zeros((0, 5, 3)), np.zeros((4, 5, 3), dtype=complex)):
        with pytest.raises(ValueError):
            mg.update(block)
    assert mg._h is None and mg.n_draws == 0
    if la.device_count() == 0:
        with pytest.raises(la.LogregHipError, match="no CPU fallback"):
            mg.update(np.zeros((4, 5, 3)))
    # mcmc(marginals=): keyword-only, ahead of predictive (which stays last), refused with a reason before anything runs
    params = inspect.signature(la.mcmc).parameters
    par = params["marginals"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert list(params)[-1] == "predictive" and list(params)[-2] == "marginals"
    with pytest.raises(ValueError, match="needs a fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, marginals=la.Marginals(1, 2, lo=[0, 0], hi=[1, 1]))
    import twin
    from logreg_amd import _lib
    X, y = pima
    L = twin.install()
    try:
        assert _lib.load() is L and not hasattr(L, "lr_marg_create")
        model = la.LogReg(X, y, pscale, dtype="float64")
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.zeros((6, 8))
        lo8, hi8 = -np.ones(8), np.ones(8)
        for wrong in (la.Marginals(5, 8, "float64", lo8, hi8), la.Marginals(6, 7, "float64", lo8[:7], hi8[:7]), la.Marginals(6, 8, "float32", lo8, hi8),
                      la.Marginals(6, 8, "float64", lo8, hi8, device=1)):
            with pytest.raises(ValueError, match="marginals= is for"):
                la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, marginals=wrong)
        with pytest.raises(ValueError, match="must be a Marginals"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, marginals="yes")
        with pytest.raises(la.LogregHipError, match="no marginals entry points"):  # a library without the new header says so
            la.Marginals(6, 8, "float64", lo8, hi8).update(np.zeros((2, 6, 8)))
        model.close()
    finally:
        twin.uninstall()
