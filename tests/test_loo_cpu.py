"""PSIS-LOO (include/logreg_hip_loo.h, logreg_amd/loo.py) -- everything that can be checked without a GPU: the reference's closed form
against the direct log-sum-exp form, the tail length in integers, the NumPy summaries, argument validation, the ABI tables and the
build gates with the new kernels in both libraries."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import loo_cases as lc
import loo_reference as lref

WANT = ["lr_loo_accumulate", "lr_loo_create", "lr_loo_destroy", "lr_loo_loglik", "lr_loo_reset", "lr_loo_result", "lr_psis"]
_SEEN = {}


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


@pytest.mark.parametrize("name", lc.CLOSED_FORM_NAMES)
def test_closed_form_elpd_agrees_with_the_direct_log_sum_exp_form(name):
    """The body draws all have weight x likelihood = e^-a, which is what lets the kernel skip the map from the sorted tail back to the
    draws.  Bound 1e-13 absolute (the issue's; measured 2e-15)."""
    c = lc.model_case(name)
    L = lref.loglik_matrix(*lc.rounded(c, np.float64))
    worst, khats = 0.0, []
    for i in range(L.shape[1]):
        out, lw = lref.psis_row(L[:, i], return_lw=True)
        worst = max(worst, abs(out[0] - lref.direct_elpd(L[:, i], lw)))
        khats.append(out[1])
    print(f"[loo] closed form vs direct, {name}: {worst:.3e}")
    assert worst <= 1e-13, (name, worst)
    _SEEN[name] = np.array(khats)


def test_the_psis_case_list_spans_negative_high_and_very_high_khat():
    """On the reference side: the GPU test's inputs really contain k-hat < 0, > 0.7 and > 1, and rows on both sides of 0.7."""
    tabs = {}
    for name in lc.PSIS_NAMES:
        if name not in _SEEN:
            c = lc.model_case(name)
            _SEEN[name] = lref.psis_table(lref.loglik_matrix(*lc.rounded(c, np.float64)))[1]
        tabs[name] = _SEEN[name]
    allk = np.concatenate(list(tabs.values()))
    print("[loo] khat range", float(np.min(allk)), float(np.max(allk[np.isfinite(allk)])), {k: int(np.sum(v > 0.7)) for k, v in tabs.items()})
    assert np.any(allk < 0) and np.any((allk > 0.7) & np.isfinite(allk)) and np.any((allk > 1) & np.isfinite(allk))
    assert np.sum(tabs["pima_S25"] > 0.7) > 0 and np.sum(tabs["synthetic_n60_p32_S4096"] > 0.7) > 0
    assert np.sum(tabs["synthetic_n300_p3_S4096"] > 0.7) == 0


def test_tail_length_and_cutoff_index_in_integers():
    from logreg_amd.loo import tail_length
    for S, M in lc.TAIL_LENGTHS.items():
        assert tail_length(S) == lref.tail_length(S) == M, S
        m3 = next(m for m in range(0, 4000) if m * m >= 9 * S)
        assert M == min(S // 5, m3)
        if M:
            v = -np.arange(S, dtype=np.float64)  # distinct: the tail is exactly the M largest
            out = lref.psis_row(-v - 3.0)
            assert out[4] == (M if M >= 1 else 0)
            assert np.sort(v)[S - M - 1] == v[M]  # ascending index S - M - 1 is the (M + 1)-th largest
    hdr = open(os.path.join(REPO, "include", "logreg_hip_loo.h")).read()
    from logreg_amd import _lib
    cap = int(re.search(r"#define LR_LOO_MAX_DRAWS (\d+)", hdr).group(1))
    assert cap == _lib.LOO_MAX_DRAWS == 1 << 20 and tail_length(cap) == 3072 and tail_length(cap + 1) == 3073
    assert _lib.LOO_ROWS == int(re.search(r"#define LR_LOO_ROWS (\d+)", hdr).group(1)) == 5


def test_reference_on_hand_made_columns():
    S = 100
    const = np.full(S, -0.7)
    e, k, ne, lp, nt = lref.psis_row(const)
    assert (e, k, nt) == (-0.7, np.inf, 0.0) and abs(ne - S) < 1e-12 and abs(lp + 0.7) < 1e-15
    rng = np.random.default_rng(0)
    l24, l25 = -rng.exponential(size=24), -rng.exponential(size=25)
    assert lref.psis_row(l24)[1] == np.inf and lref.psis_row(l24)[4] == 4  # M = 4: raw weights
    o25 = lref.psis_row(l25)
    assert np.isfinite(o25[1]) and o25[4] == 5  # M = 5: smoothed
    tied = l25.copy()
    order = np.argsort(tied)  # ascending l = descending v; make the cutoff value occur inside the would-be tail too
    tied[order[3:6]] = tied[order[5]]
    o = lref.psis_row(tied)
    assert 0 < o[4] < 5 and o[1] == np.inf  # ties at the cutoff shrink the tail to 3 <= 4
    assert all(np.isnan(lref.psis_row(np.where(np.arange(S) == 7, np.nan, const))))


def test_loo_from_table_and_loo_compare_arithmetic():
    from logreg_amd import loo_compare, loo_from_table
    t = np.array([[-0.5, -1.0, -2.5], [0.1, 0.8, np.inf], [90.0, 40.0, 3.0], [-0.4, -0.7, -1.5], [19.0, 19.0, 4.0]])
    r = loo_from_table(t, 100)
    assert r["elpd_loo"] == -4.0 and r["looic"] == 8.0 and abs(r["p_loo"] - 1.4) < 1e-15 and r["n_draws"] == 100
    assert abs(r["se"] - np.sqrt(3 * np.var([-0.5, -1.0, -2.5], ddof=1))) < 1e-15 and r["n_khat_over_0_7"] == 2
    assert np.array_equal(r["khat"], t[1]) and np.array_equal(r["n_tail"], t[4]) and np.array_equal(r["n_eff"], t[2])
    t2 = t.copy()
    t2[0] = [-0.6, -0.8, -2.0]
    c = loo_compare(r, loo_from_table(t2, 50))
    d = np.array([0.1, -0.2, -0.5])
    assert abs(c["elpd_diff"] - d.sum()) < 1e-15 and abs(c["se_diff"] - np.sqrt(3 * np.var(d, ddof=1))) < 1e-15 and c["n"] == 3
    with pytest.raises(ValueError, match="same observations"):
        loo_compare(r, loo_from_table(t[:, :2], 100))
    with pytest.raises(ValueError):
        loo_from_table(t[:4], 100)
    nan = loo_from_table(np.full((5, 3), np.nan), 0)
    assert np.isnan(nan["elpd_loo"]) and nan["n_khat_over_0_7"] == 0


def test_symbol_table_matches_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_loo.h") == WANT == sorted(_lib.LOO_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS):
        assert not set(WANT) & set(other)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38  # logreg_hip.h's set stays as pinned
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_loo_\w+|lr_psis\w*)", exported))) == WANT, path
    assert _lib.load_loo() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_loo.h") in src and os.path.join(build.CSRC, "lr_loo.h") in src


def test_still_13_units_and_the_loo_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_loo_" in r["name"] or "k_psis" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32, 64, 128):
                assert sum(f"k_loo_fill<{dt}, {P}>" in r["name"] for r in mine) == 1, (alt, dt, P)
            assert sum(f"k_loo_transpose<{dt}>" in r["name"] for r in mine) == 1
            assert sum(f"k_psis<{dt}, 256, 1024, 1024>" in r["name"] for r in mine) == 1 and sum(f"k_psis<{dt}, 512, 4096, 3072>" in r["name"] for r in mine) == 1
        assert len(mine) == 18
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert all(r["lds"] <= 64 * 1024 for r in mine)
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


def test_no_gpu_means_loud_failure_not_fallback():
    import logreg_amd as la
    if la.device_count() > 0:  # with a device the same calls get as far as their argument checks
        with pytest.raises(TypeError):
            la.PsisLoo(None, 10)
        return
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.PsisLoo(None, 10)
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.psis_loo(None, np.zeros((4, 8)))
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.psis_from_loglik(np.zeros((30, 2)))


def test_shape_and_type_refusals_of_the_python_face(pima, pscale):
    """On tests/twin.py (a library without the PSIS-LOO entry points): the Python face validates its arguments before it needs the
    library, says so when the library has no such entry points, and mcmc refuses a wrong loo= before anything runs."""
    import logreg_amd as la
    from logreg_amd import _lib
    import twin
    params = inspect.signature(la.mcmc).parameters
    assert params["loo"].kind is inspect.Parameter.KEYWORD_ONLY and params["loo"].default is None
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, loo=object())
    X, y = pima
    L = twin.install()
    try:
        assert _lib.load() is L and not hasattr(L, "lr_loo_create")
        model = la.LogReg(X, y, pscale, dtype="float64")
        with pytest.raises(TypeError, match="LogReg"):
            la.PsisLoo("model", 10)
        with pytest.raises(TypeError, match="integer"):
            la.PsisLoo(model, 10.5)
        for bad in (0, -3):
            with pytest.raises(ValueError, match="positive"):
                la.PsisLoo(model, bad)
        with pytest.raises(la.LogregHipError, match="no PSIS-LOO entry points"):
            la.PsisLoo(model, 10)
        with pytest.raises(la.LogregHipError, match="no PSIS-LOO entry points"):
            la.psis_from_loglik(np.zeros((30, 2)))
        with pytest.raises(ValueError, match=r"\[S, p\]"):
            la.psis_loo(model, np.zeros(8))
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        with pytest.raises(ValueError, match="must be a PsisLoo"):
            la.mcmc(np.zeros((6, 8)), kern, thin=1, iters=2, verb=False, seed=1, loo="yes")
        # an accumulator of another model, and one that is too small: built by hand, since this library cannot make one
        other = la.LogReg(X, y, pscale, dtype="float32")
        fake = object.__new__(la.PsisLoo)
        fake._h, fake.model, fake.max_draws, fake.n_draws, fake.n = None, other, 100, 0, other.n
        with pytest.raises(ValueError, match="own model"):
            la.mcmc(np.zeros((6, 8)), kern, thin=1, iters=2, verb=False, seed=1, loo=fake)
        fake.model, fake.max_draws, fake.n_draws = model, 12, 1
        with pytest.raises(ValueError, match="max_draws = 12"):
            la.mcmc(np.zeros((6, 8)), kern, thin=1, iters=2, verb=False, seed=1, loo=fake)
        for draws in (np.zeros((4, 7)), np.zeros((0, 8)), np.zeros((2, 3, 4, 8))):
            with pytest.raises(ValueError):
                fake.update(draws)
        with pytest.raises(ValueError, match="exceed max_draws"):
            fake.update(np.zeros((12, 8)))
        other.close()
        model.close()
    finally:
        twin.uninstall()
