"""Autocorrelation / Geyer ESS on the device (include/logreg_hip_acf.h, logreg_amd/autocorr.py) -- everything that can be checked without
a GPU: the ABI tables, the build gates with the new kernels in both builds, the independent reference against the project's host
estimator, the margin condition of the test set, the NumPy merge, and argument validation ahead of any device access."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import acf_cases as cases
import acf_reference as ar

WANT = ["lr_acf_accumulate", "lr_acf_create", "lr_acf_destroy", "lr_acf_reset", "lr_acf_result"]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_acf.h") == WANT == sorted(_lib.ACF_SYMBOLS)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_acf_\w+)", exported))) == WANT, path
    hdr = open(os.path.join(REPO, "include", "logreg_hip_acf.h")).read()
    assert _lib.ACF_MAX_LAG == int(re.search(r"#define LR_ACF_MAX_LAG (\d+)", hdr).group(1)) == 255
    assert re.search(r"#define LR_ACF_ROWS\(K\) \(\(K\) \+ (\d+)\)", hdr).group(1) == str(_lib.ACF_HEAD_ROWS + 1)
    assert _lib.load_acf() is _lib.load()  # binds on first use


def test_the_older_symbol_sets_are_unchanged():
    from logreg_amd import _lib
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    assert _declared("logreg_hip_nuts.h") == sorted(_lib.NUTS_SYMBOLS) == ["lr_run_nuts"]
    assert _declared("logreg_hip_predict.h") == sorted(_lib.PREDICT_SYMBOLS) == [
        "lr_predict_accumulate", "lr_predict_create", "lr_predict_destroy", "lr_predict_reset", "lr_predict_result"]
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS):
        assert not set(WANT) & set(other)
    assert not any(s.startswith(("lr_predict_", "lr_run_")) for s in WANT)


def test_header_and_kernels_are_part_of_the_build_id():
    from logreg_amd import build
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_acf.h") in src and os.path.join(build.CSRC, "lr_acf.h") in src


def test_still_13_units_and_the_acf_kernels_pass_both_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_acf_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):  # both dtypes x one to four lags per lane
            for nl in (1, 2, 3, 4):
                assert sum(f"k_acf_accumulate<{dt}, {nl}>" in r["name"] for r in mine) == 1, (alt, dt, nl)
        for k in ("k_acf_finish", "k_acf_partial", "k_acf_final"):
            assert sum(k in r["name"] for r in mine) == 1, (alt, k)
        assert len(mine) == 11
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)  # (the second build may use scratch in older kernels: its gate only reports)


def test_reference_is_the_hosts_estimator_where_no_series_is_capped():
    """acf_reference shares nothing with diagnostics.ess_geyer (direct long-double sums against an FFT), and agrees with it to 1e-9
    relative on every uncapped finite series; the sum over chains is ess_pooled(max_chains=None)."""
    from logreg_amd import diagnostics as dg
    seen = 0
    for name in ("C37_p8_n64_K63", "C5_p20_n200_K63", "C5_p3_n601_K255", "C1_p8_n601_K255", "C5_p3_n5_K7", "C5_p3_n8_K7", "C1_p3_n3_K7"):
        for dtype in cases.DTYPES:
            c = cases.case(name, dtype)
            ref = ar.reference(c["x"], c["K"])
            for ch in range(c["C"]):
                for j in range(c["p"]):
                    if ref["nan"][ch, j] or ref["capped"][ch, j]:
                        continue
                    host = dg.ess_geyer(c["x"][:, ch, j])
                    assert abs(ref["ess"][ch, j] - host) <= 1e-9 * abs(host), (name, dtype, ch, j, ref["ess"][ch, j], host)
                    seen += 1
            if not ref["nan"].any() and not ref["capped"].any():
                pooled = dg.ess_pooled(c["x"], max_chains=None)
                assert np.all(np.abs(ref["sums"][0] - pooled) <= 1e-9 * pooled), (name, dtype)
    assert seen > 500
    c = cases.case("C1_p8_n601_K255", "float64")  # no special series: the pooled identity is exercised
    assert not ar.reference(c["x"], c["K"])["capped"].any()


def test_capped_series_exist_and_use_every_pair():
    c = cases.case("C37_p1_n601_K63", "float64")
    ref = ar.reference(c["x"], 63)
    full = ar.reference(c["x"], 255)
    assert ref["capped"].sum() >= 3 and not full["capped"].any()
    assert np.all(ref["trunc"][ref["capped"]] == 32) and np.all(full["trunc"][ref["capped"]] > 32)
    assert np.all(ref["ess"][ref["capped"]] > full["ess"][ref["capped"]])  # fewer positive pairs: a smaller tau
    assert np.array_equal(ref["sums"][1], ref["capped"].sum(axis=0).astype(float))


@pytest.mark.parametrize("name", cases.NAMES)
def test_margin_condition_holds_for_every_series_of_the_set(name):
    """The truncation index is discontinuous in Gamma: every scanned series keeps |Gamma_j| >= 1e3 x its bound up to and including its
    truncation pair (and |tau| >= 1e3 x its bound), so the kernel and the reference take the same branch."""
    for dtype in cases.DTYPES:
        c = cases.case(name, dtype)
        ref = ar.reference(c["x"], c["K"])
        m = ref["margin"]
        assert np.array_equal(np.isnan(m), ref["nan"])
        assert np.nanmin(m) >= 1e3 if m.size else True, (name, dtype, float(np.nanmin(m)))
        if c["C"] >= 5:  # the special series are there: constant -> ESS = n exactly, NaN / inf -> counted
            assert ref["ess"][1, 0] == c["n"] and ref["tol_ess"][1, 0] == 0 and np.all(ref["acov"][:, 1, 0] == 0)
            assert ref["nan"][3, 0] and ref["nan"][4, c["p"] - 1] and ref["sums"][2].sum() == ref["nan"].sum() >= 2
            assert np.isnan(ref["sums"][0, 0]) and np.isnan(ref["sums"][3, 0])


def test_merge_autocorr_of_two_halves_is_the_whole():
    from logreg_amd import merge_autocorr
    from logreg_amd.autocorr import result_from_sums
    c = cases.case("C37_p8_n64_K63", "float64")
    x = np.array(c["x"])
    x[:, 3, 0] = x[:, 5, 0]  # (finite everywhere: every entry can be compared)
    x[:, 4] = x[:, 6]
    whole = ar.reference(x, 63)
    parts = [ar.reference(x[:, :20], 63), ar.reference(x[:, 20:], 63)]
    res = merge_autocorr([result_from_sums(q["sums"], q["ess"], 64, q["ess"].shape[0]) for q in parts])
    want = result_from_sums(whole["sums"], whole["ess"], 64, 37)
    assert res["chains"] == 37 and res["n"] == 64 and res["max_lag"] == 63
    assert np.array_equal(res["ess_chain"], whole["ess"]) and np.array_equal(res["capped"], want["capped"])
    for key in ("ess", "acf", "ess_pooled_acf", "mcse", "sums"):
        assert np.allclose(res[key], want[key], rtol=1e-12, atol=1e-15), key
    assert res["acf"].shape == (64, 8) and np.all(res["acf"][0] == 1.0) and np.all(res["ess_pooled_acf"] > 0)
    with pytest.raises(ValueError):
        merge_autocorr([])
    with pytest.raises(ValueError):
        merge_autocorr([want, result_from_sums(whole["sums"], whole["ess"], 65, 37)])


def test_autocorr_validates_before_any_device_access(pima, pscale):
    import logreg_amd as la
    for bad in (dict(max_lag=64), dict(max_lag=0), dict(max_lag=257), dict(dtype="float16"), dict(chains=0), dict(p=0), dict(dtype="int32")):
        kw = dict(chains=5, p=3, dtype="float32")
        kw.update(bad)
        with pytest.raises(ValueError):
            la.Autocorr(**kw)
    ac = la.Autocorr(5, 3, "float64")  # no device yet: nothing is allocated before the first block
    assert ac.max_lag == 63 and ac.n_draws == 0 and ac.dtype == np.float64 and ac._h is None
    for block in (np.zeros((4, 5)), np.zeros((4, 3, 5)), np.zeros((4, 5, 4)), np.zeros((0, 5, 3)), np.zeros((4, 5, 3), dtype=complex)):
        with pytest.raises(ValueError):
            ac.update(block)
    assert ac._h is None and ac.n_draws == 0
    if la.device_count() == 0:
        with pytest.raises(la.LogregHipError, match="no CPU fallback"):
            ac.update(np.zeros((4, 5, 3)))
    # mcmc(autocorr=): keyword-only, refused with a reason before anything runs
    par = inspect.signature(la.mcmc).parameters["autocorr"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, autocorr=la.Autocorr(1, 2))
    import twin
    from logreg_amd import _lib
    X, y = pima
    L = twin.install()
    try:
        assert _lib.load() is L and not hasattr(L, "lr_acf_create")
        model = la.LogReg(X, y, pscale, dtype="float64")
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.zeros((6, 8))
        for wrong in (la.Autocorr(5, 8, "float64"), la.Autocorr(6, 7, "float64"), la.Autocorr(6, 8, "float32"), la.Autocorr(6, 8, "float64", device=1)):
            with pytest.raises(ValueError, match="autocorr= is for"):
                la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, autocorr=wrong)
        with pytest.raises(ValueError, match="must be an Autocorr"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, autocorr="yes")
        with pytest.raises(la.LogregHipError, match="no autocorrelation entry points"):  # a library without the new header says so
            la.Autocorr(6, 8, "float64").update(np.zeros((2, 6, 8)))
        model.close()
    finally:
        twin.uninstall()
