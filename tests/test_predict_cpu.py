"""Posterior prediction / WAIC (include/logreg_hip_predict.h, logreg_amd/predict.py) -- everything that can be checked without a GPU:
the ABI tables, the build gates with the new kernels in the library, the reference's own guard, the NumPy merge, the WAIC arithmetic,
argument validation, and that the test doubles of the older ABI tables keep working beside the new one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import predict_reference as pr


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def _case(r=37, p=5, S=300, seed=1):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(r), rng.standard_normal((r, p - 1))])
    beta = rng.standard_normal(p) * 0.8
    y = (rng.random(r) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    B = beta[None, :] + 0.3 * rng.standard_normal((S, p))
    return X, y, B


def test_symbol_tables_match_the_header_and_the_library():
    from logreg_amd import _lib, build
    want = ["lr_predict_accumulate", "lr_predict_create", "lr_predict_destroy", "lr_predict_reset", "lr_predict_result"]
    assert _declared("logreg_hip_predict.h") == want == sorted(_lib.PREDICT_SYMBOLS)
    assert not set(want) & set(_lib.SYMBOLS) and not set(want) & set(_lib.NUTS_SYMBOLS)  # logreg_hip.h's set stays as pinned
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in want:
            assert hasattr(L, s), (path, s)
    exported = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    assert sorted(set(re.findall(r"\b(lr_predict_\w+)", exported))) == want
    assert _lib.PRED_ROWS == int(re.search(r"#define LR_PRED_ROWS (\d+)", open(os.path.join(REPO, "include", "logreg_hip_predict.h")).read()).group(1))
    assert _lib.load_predict() is _lib.load()  # binds on first use


def test_header_is_part_of_the_build_id():
    from logreg_amd import build
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_predict.h") in src and os.path.join(build.CSRC, "lr_predict.h") in src


def test_still_13_units_no_scratch_no_exec_findings_and_the_predict_kernels_are_there():
    from logreg_amd import build as b, isa_gate
    b.build(verbose=False)
    objs = b.unit_objects()
    assert len(objs) == 13
    rows = b.kernel_resources()
    mine = [r for r in rows if "k_predict" in r["name"]]
    # float32 / float64 x six padded widths x with / without labels, the merge, two padding kernels -- all in the C-ABI unit
    assert len([r for r in mine if "k_predict_partial" in r["name"]]) == 24 and {r["unit"] for r in mine} == {"lr_api"}
    assert any("k_predict_merge" in r["name"] for r in mine) and sum("k_predict_pad" in r["name"] for r in mine) == 2
    for dt in ("float", "double"):
        for P in (4, 8, 16, 32, 64, 128):
            assert sum(f"k_predict_partial<{dt}, {P}," in r["name"] for r in mine) == 2, (dt, P)
    assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
    b.resource_gate(strict=True, verbose=False)
    assert isa_gate.scan_paths(objs) == []
    b.exec_prologue_gate(strict=True, verbose=False)


def test_reference_guards_itself_against_library_functions():
    X, y, B = _case()
    ref, info = pr.reference_table(X, y, B, return_info=True)
    brute = pr.brute_force_table(X, y, B)
    assert ref.shape == brute.shape == (5, 37) and info["min_L"] > 1e-6
    for row in (0, 2, 3):
        assert np.max(np.abs(ref[row] - brute[row])) < 2e-15, row
    for row in (1, 4):
        assert np.max(np.abs(ref[row] - brute[row]) / brute[row]) < 1e-11, row
    # row blocking does not change a bit; a [iters, C, p] block is the same draws
    assert np.array_equal(ref, pr.reference_table(X, y, B, block_pairs=1000))
    assert np.array_equal(ref, pr.reference_table(X, y, B.reshape(30, 10, -1)))
    nolab = pr.reference_table(X, None, B)
    assert np.array_equal(nolab[:2], ref[:2]) and np.all(np.isnan(nolab[2:]))
    # the float32 mode differs from the float64 one at float32's scale, not more and not zero
    X32, B32 = X.astype(np.float32), B.astype(np.float32)
    d = np.abs(pr.reference_table(X32, y, B32, mode="float32") - pr.reference_table(X32.astype(float), y, B32.astype(float)))
    assert 0 < d[0].max() < 1e-6 and 0 < d[3].max() < 1e-5


def test_row_2_is_not_one_minus_row_0_where_it_matters():
    """Why the table keeps mean L beside mean pi: for a confidently and rightly predicted y = 0 row, 1 - mean(pi) is L; for a tiny L
    (a confidently WRONG prediction) 1 - mean(pi) has lost it."""
    X = np.array([[1.0, 40.0]])
    B = np.array([[0.0, 1.0], [0.0, 1.01]])
    t = pr.reference_table(X, np.array([0.0]), B)
    assert 0 < t[2, 0] < 1e-17 and 1.0 - t[0, 0] == 0.0


def test_merge_predictive_of_any_split_equals_the_whole_run():
    from logreg_amd import merge_predictive
    X, y, B = _case(r=23, p=4, S=1000, seed=7)
    whole = pr.reference_table(X, y, B)
    rng = np.random.default_rng(3)
    for cuts in ([500], [1], [999], [10, 11, 700], sorted(rng.choice(np.arange(1, 1000), 9, replace=False))):
        edges = [0, *cuts, 1000]
        parts = [B[a:b] for a, b in zip(edges, edges[1:])]
        tabs = [pr.reference_table(X, y, q) for q in parts]
        tab, n = merge_predictive(tabs, [len(q) for q in parts])
        assert n == 1000
        for row in (0, 2, 3):
            assert np.max(np.abs(tab[row] - whole[row])) < 1e-14, (cuts, row)
        for row in (1, 4):
            assert np.max(np.abs(tab[row] - whole[row]) / whole[row]) < 1e-12, (cuts, row)
    # empty shards are skipped, a single table comes back as it is, shapes and counts are checked
    tab, n = merge_predictive([np.full((5, 23), np.nan), whole], [0, 1000])
    assert n == 1000 and np.array_equal(tab, whole)
    with pytest.raises(ValueError):
        merge_predictive([whole], [1, 2])
    with pytest.raises(ValueError):
        merge_predictive([whole, whole[:, :5]], [1, 2])
    with pytest.raises(ValueError):
        merge_predictive([whole[:4]], [1])
    # without labels rows 2 - 4 stay NaN
    nolab = [pr.reference_table(X, None, q) for q in (B[:300], B[300:])]
    tab, _ = merge_predictive(nolab, [300, 700])
    assert np.all(np.isnan(tab[2:])) and np.max(np.abs(tab[0] - whole[0])) < 1e-14


def test_waic_arithmetic_from_a_hand_made_table():
    from logreg_amd import waic_from_table
    S = 11
    table = np.array([[0.5, 0.25, 0.75], [0.1, 0.2, 0.3], [0.5, 0.25, 0.125], [-0.7, -1.4, -2.1], [1.0, 2.0, 4.0]])
    w = waic_from_table(table, S)
    lppd = np.log([0.5, 0.25, 0.125])
    pw = np.array([0.1, 0.2, 0.4])
    elpd_i = lppd - pw
    assert np.allclose(w["lppd_i"], lppd, rtol=0, atol=1e-15) and np.allclose(w["p_waic_i"], pw, rtol=0, atol=1e-15)
    assert abs(w["elpd_waic"] - elpd_i.sum()) < 1e-14 and abs(w["p_waic"] - 0.7) < 1e-14 and abs(w["waic"] + 2 * elpd_i.sum()) < 1e-14
    assert abs(w["se"] - np.sqrt(3 * np.var(elpd_i, ddof=1))) < 1e-14 and w["n_draws"] == S
    with pytest.raises(ValueError, match="two draws"):
        waic_from_table(table, 1)
    nolab = table.copy()
    nolab[2:] = np.nan
    with pytest.raises(ValueError, match="labels"):
        waic_from_table(nolab, S)
    with pytest.raises(ValueError):
        waic_from_table(table[:3], S)


def test_no_gpu_means_loud_failure_not_fallback(pima):
    import logreg_amd as la
    X, y = pima
    if la.device_count() > 0:  # with a device the same call gets as far as its argument check
        with pytest.raises(TypeError):
            la.PosteriorPredictive(None)
        return
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.PosteriorPredictive(None)
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.predict_proba(None, np.zeros((4, 8)), X)
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.waic(None, np.zeros((4, 8)))


def test_mcmc_refuses_predictive_with_a_generic_kernel():
    import logreg_amd as la
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, predictive=object())
    import inspect
    assert list(inspect.signature(la.mcmc).parameters)[-1] == "predictive" and inspect.signature(la.mcmc).parameters["predictive"].default is None


def test_twins_still_install_and_argument_validation_on_the_twin(pima, pscale):
    """tests/twin.py and tests/twin_nuts.py bind SYMBOLS / NUTS_SYMBOLS onto libraries without the prediction entry points: they install as
    before; the Python face validates its arguments before it needs the library, and says so when the library has no such entry points."""
    import logreg_amd as la
    from logreg_amd import _lib
    import twin
    import twin_nuts
    X, y = pima
    for mod in (twin, twin_nuts):
        L = mod.install()
        try:
            assert _lib.load() is L and not hasattr(L, "lr_predict_create")
            model = la.LogReg(X, y, pscale, dtype="float64")
            assert np.isfinite(model.lpost(np.zeros(8)))
            with pytest.raises(TypeError):
                la.PosteriorPredictive("model")
            with pytest.raises(ValueError, match=r"\[r, p\]"):
                la.PosteriorPredictive(model, X[:, :5])
            with pytest.raises(ValueError, match="no rows"):
                la.PosteriorPredictive(model, X[:0])
            with pytest.raises(ValueError, match="finite"):
                la.PosteriorPredictive(model, np.where(np.arange(8) == 3, np.nan, X[:4]))
            with pytest.raises(ValueError, match="0 / 1"):
                la.PosteriorPredictive(model, X[:4], [0, 1, 2, 1])
            with pytest.raises(ValueError, match=r"\[r\]"):
                la.PosteriorPredictive(model, X[:4], [0, 1, 1])
            with pytest.raises(ValueError, match="without X_new"):
                la.PosteriorPredictive(model, None, y)
            with pytest.raises(la.LogregHipError, match="prediction entry points"):
                la.PosteriorPredictive(model)
            model.close()
        finally:
            mod.uninstall()
