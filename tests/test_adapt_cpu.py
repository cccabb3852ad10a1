"""The NUTS warm-up (include/logreg_hip_adapt.h, logreg_amd/adapt.py) -- everything that can be checked without a GPU: the schedule of the
library against the hand-listed window ends and against the NumPy restatement (tests/adapt_reference.py), the ABI tables, the build
gates with the new kernels in both builds, the reference's dual averaging against a hand-computed sequence, the four mutations that the
teacher-forced comparison of tests/test_gpu_adapt.py must reject at its own tolerance (on a device trace recorded under tests/golden/),
argument validation ahead of any device access, and the host side of the handle (tests/host/adapt_harness.cpp, a stand-alone program)
under AddressSanitizer and UBSan."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import host_build
import adapt_cases as cases
import adapt_reference as ar

WANT = ["lr_adapt_create", "lr_adapt_destroy", "lr_adapt_result", "lr_adapt_run", "lr_adapt_schedule", "lr_adapt_trace"]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def _lib_schedule(L, W, init=0, term=0, base=0):
    ends = (ctypes.c_int32 * 32)()
    n, first = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.lr_adapt_schedule(W, init, term, base, ends, ctypes.byref(n), ctypes.byref(first)) == 0
    return first.value, list(ends[:n.value])


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_adapt.h") == WANT == sorted(_lib.ADAPT_SYMBOLS)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS):
        assert not set(WANT) & set(other)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_adapt_\w+)", exported))) == WANT, path
    hdr = open(os.path.join(REPO, "include", "logreg_hip_adapt.h")).read()
    assert _lib.ADAPT_MAX_WINDOWS == int(re.search(r"#define LR_ADAPT_MAX_WINDOWS (\d+)", hdr).group(1))
    assert _lib.ADAPT_TRACE_COLS == int(re.search(r"#define LR_ADAPT_TRACE_COLS (\d+)", hdr).group(1))
    assert _lib.ADAPT_ITER_BASE == 2 ** 62 and "INT64_C(1) << 62" in hdr
    assert ctypes.sizeof(_lib.AdaptOpts) == 72 and ctypes.sizeof(_lib.AdaptInfo) == 24
    assert _lib.load_adapt() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_adapt.h") in src and os.path.join(build.CSRC, "lr_adapt.h") in src


def test_still_13_units_and_the_warmup_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        rows = b.kernel_resources(alt=alt)
        mine = [r for r in rows if "k_adapt_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"} and len(mine) == 16
        tuned = [r for r in rows if "k_nuts<" in r["name"] and ", true>" in r["name"]]
        plain = [r for r in rows if "k_nuts<" in r["name"] and ", false>" in r["name"]]
        assert len(tuned) == 8 == len(plain) and {r["unit"] for r in tuned} == {r["unit"] for r in plain}
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32):
                for k in ("k_adapt_partial", "k_adapt_update"):
                    assert sum(f"{k}<{dt}, {P}>" in r["name"] for r in mine) == 1, (alt, k, dt, P)
                assert sum(f"k_nuts<{dt}, {P}, 1, 0, true>" in r["name"] for r in tuned) == 1, (alt, dt, P)
        new = mine + tuned
        assert all(r["scratch"] == 0 for r in new), [(r["name"], r["scratch"]) for r in new if r["scratch"]]
        assert all(r["lds"] <= 4096 for r in mine)
        key = lambda r: re.search(r"k_nuts<(\w+), (\d+)", r["name"]).groups()  # noqa: E731
        lds = {key(r): r["lds"] for r in tuned}
        for r in plain:  # the tuned kernel is planned as the plain one: the same static LDS
            assert lds[key(r)] == r["lds"]
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


def test_schedule_of_the_library_is_the_hand_listed_one_and_the_references():
    from logreg_amd import _lib
    from logreg_amd.adapt import adapt_schedule
    L = _lib.load_adapt()  # (host code: needs no device)
    for W, (init, ends) in cases.HAND_SCHEDULE.items():
        assert _lib_schedule(L, W) == (init, ends) == ar.schedule(W), W
        assert adapt_schedule(W) == (init, ends)
    for W in list(range(1, 301)) + [1000]:
        assert _lib_schedule(L, W) == ar.schedule(W), W
        for buf in ((10, 5, 7), (1, 1, 1), (100, 100, 100), (20, 30, 5), (75, 50, 24)):
            got, want = _lib_schedule(L, W, *buf), ar.schedule(W, *buf)
            assert got == want, (W, buf, got, want)
            first, ends = got
            assert all(a < b for a, b in zip([first] + ends, ends)) and (not ends or ends[-1] <= W)
    ends = (ctypes.c_int32 * 32)()
    n = ctypes.c_int32()
    for bad in ((0, 0, 0, 0), (-5, 0, 0, 0), (100, -1, 0, 0), (100, 0, -1, 0), (100, 0, 0, -1)):
        assert L.lr_adapt_schedule(*bad, ends, ctypes.byref(n), None) == -1
        assert b"lr_adapt_schedule" in L.lr_last_error()
    assert L.lr_adapt_schedule(100, 0, 0, 0, None, ctypes.byref(n), None) == -1


def test_reference_dual_averaging_against_a_hand_computed_sequence():
    """Three steps from eps0 = 1, delta 0.8, gamma 0.05, t0 10, kappa 0.75 on abar = 1, 0.5, 0, worked by hand:
    mu = ln 10.  m = 1: Hbar = (0.8 - 1) / 11 = -1/55; ln eps = ln 10 + 20 / 55; eta = 1: ln eps_bar = ln eps.
    m = 2: Hbar = (11/12)(-1/55) + 0.3 / 12 = -1/60 + 1/40 = 1/120; ln eps = ln 10 - 20 sqrt 2 / 120.
    m = 3: Hbar = (12/13)(1/120) + 0.8 / 13 = 1/130 + 8/130 = 9/130; ln eps = ln 10 - 20 sqrt 3 * 9 / 130."""
    d = ar.dual_averaging([1.0, 0.5, 0.0])
    l10, r2, r3 = np.log(10.0), np.sqrt(2.0), np.sqrt(3.0)
    le = [l10 + 20.0 / 55.0, l10 - 20.0 * r2 / 120.0, l10 - 20.0 * r3 * 9.0 / 130.0]
    assert d["eps"][0] == 1.0
    np.testing.assert_allclose(d["eps"][1:], np.exp(le[:2]), rtol=1e-14)
    assert d["next"] == pytest.approx(np.exp(le[2]), rel=1e-14)
    e2, e3 = 2.0 ** -0.75, 3.0 ** -0.75
    leb = [le[0]]
    leb.append(e2 * le[1] + (1 - e2) * leb[0])
    leb.append(e3 * le[2] + (1 - e3) * leb[1])
    np.testing.assert_allclose(d["log_eps_bar"], leb, rtol=1e-14)
    assert d["final"] == pytest.approx(np.exp(leb[2]), rel=1e-14)
    # a restart after the second step: mu = ln(10 eps), Hbar = 0, ln eps_bar = 0, m = 0
    r = ar.dual_averaging([1.0, 0.5, 0.0], restarts=[1])
    eps2 = np.exp(le[1])
    assert r["eps"][2] == pytest.approx(eps2, rel=1e-14)
    assert r["next"] == pytest.approx(np.exp(np.log(10 * eps2) - 20.0 * (0.8 / 11.0)), rel=1e-14)
    assert r["log_eps_bar"][2] == pytest.approx(np.log(10 * eps2) - 20.0 * (0.8 / 11.0), rel=1e-14)


def test_reference_variance_and_bounds_on_known_draws():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((40, 7, 3)) * np.array([0.01, 1.0, 50.0]) + np.array([100.0, 0.0, -3.0])).astype(np.float32)
    m = ar.metric_of(x, np.ones(3))
    flat = x.reshape(-1, 3).astype(np.float64)
    N = flat.shape[0]
    var = np.var(flat, axis=0, ddof=1)
    np.testing.assert_allclose(m["var"], var, rtol=1e-12)
    np.testing.assert_allclose(m["dmm"], 1.0 / (N / (N + 5.0) * var + 1e-3 * 5.0 / (N + 5.0)), rtol=1e-12)
    assert m["n"] == N and not m["skipped"].any()
    assert np.all(m["tol_var"] < 1e-9 * m["var"]) and np.all(m["tol_dmm"] < 1e-9 * m["dmm"]) and np.all(m["tol_var"] > 0)  # tight enough to tell a wrong kernel
    x[3, 2, 1] = np.nan
    x[:, :, 2] = 4.0
    bad = ar.metric_of(x, np.array([1.0, 2.0, 3.0]))
    assert list(bad["skipped"]) == [False, True, True] and bad["dmm"][1] == 2.0 and bad["dmm"][2] == 3.0 and np.isnan(bad["var"][1]) and bad["var"][2] == 0.0
    one = ar.metric_of(x[:5, :1], np.ones(3))  # C = 1: n - 1 = window length - 1
    assert one["n"] == 5 and one["var"][0] == pytest.approx(np.var(x[:5, 0, 0].astype(np.float64), ddof=1), rel=1e-12)
    a, tol = ar.abar_of(np.full((2, 1025), 0.1))
    assert np.allclose(a, 0.1, rtol=1e-15) and np.all(tol < 1e-12)


def test_each_mutation_of_the_reference_fails_the_teacher_forced_comparison_at_the_gpu_tolerance():
    """The recorded device trace of the two-window case (tests/golden/adapt_trace_W260.json: abar_t and the step each iteration used, from
    the MI355X): the reference passes at the tolerance of tests/test_gpu_adapt.py; with t0 = 11, kappa = 0.76, m off by one, or a restart
    that keeps Hbar it must not -- otherwise the comparison proves nothing."""
    g = load_golden("adapt_trace_W260.json")
    abar, eps_dev, leb_dev = np.array(g["abar"]), np.array(g["eps"]), np.array(g["log_eps_bar"])
    W = len(abar)
    init, ends = ar.schedule(W)
    assert (init, ends) == (75, [100, 210]) and W == 260
    lasts = [e - 1 for e in ends]

    def dev(**kw):
        d = ar.dual_averaging(abar, lasts, **kw)
        return max(np.max(np.abs(d["eps"] - eps_dev) / eps_dev), np.max(np.abs(d["log_eps_bar"] - leb_dev) / np.maximum(np.abs(leb_dev), 1.0)),
                   abs(d["final"] - g["final"]) / g["final"])
    assert dev() <= cases.EPS_RTOL
    worst = {}
    for name, kw in (("t0 = 11", dict(t0=11.0)), ("kappa = 0.76", dict(kappa=0.76)), ("m off by one", dict(m_offset=1)), ("restart keeps Hbar", dict(keep_hbar=True))):
        worst[name] = dev(**kw)
        assert worst[name] > cases.EPS_RTOL, (name, worst[name])
    assert min(worst.values()) > 1e3 * cases.EPS_RTOL, worst  # not a near miss either


def test_nuts_warmup_validates_before_any_device_access(pima, pscale):
    import logreg_amd as la
    with pytest.raises(ValueError, match="needs a fused kernel"):  # the generic NumPy NUTS has no warm-up
        la.nuts_warmup(lambda b: -0.5 * np.sum(b * b), lambda b: -b, np.zeros(3), 10)
    import twin
    from logreg_amd import _lib
    from logreg_amd.adapt import adapt_schedule
    X, y = pima
    L = twin.install()
    try:
        assert _lib.load() is L and not hasattr(L, "lr_adapt_create")
        model = la.LogReg(X, y, pscale, dtype="float64")
        other = la.LogReg(X, y, pscale, dtype="float64")
        init = np.zeros((6, 8))
        with pytest.raises(ValueError, match="needs a fused kernel"):
            la.nuts_warmup(model.lpost, other.glp, init, 10)
        with pytest.raises(ValueError, match="needs a fused kernel"):
            la.nuts_warmup(model.lpost, model.lpost, init, 10)
        for bad in (dict(num_warmup=0), dict(max_depth=0), dict(max_depth=11), dict(target_accept=0.0), dict(target_accept=1.0), dict(eps=0.0), dict(eps=np.inf),
                    dict(dmm=0.0), dict(dmm=[1.0] * 7 + [np.nan]), dict(init=np.zeros((6, 7)))):
            kw = dict(init=init, num_warmup=10)
            kw.update(bad)
            with pytest.raises(ValueError):
                la.nuts_warmup(model.lpost, model.glp, **kw)
        with pytest.raises(la.LogregHipError, match="no warm-up entry points"):  # a library without the new header says so
            la.nuts_warmup(model.lpost, model.glp, init, 10)
        with pytest.raises(la.LogregHipError, match="no warm-up entry points"):
            adapt_schedule(100)
        model.close()
        other.close()
    finally:
        twin.uninstall()
    import inspect
    params = inspect.signature(la.nuts_warmup).parameters
    assert list(params) == ["lpost", "glp", "init", "num_warmup", "target_accept", "eps", "dmm", "max_depth", "adapt_metric", "seed", "chain_offset", "keep"]
    assert params["num_warmup"].default == 1000 and params["target_accept"].kind is inspect.Parameter.KEYWORD_ONLY and params["eps"].default == 1.0


def test_both_warmups_keep_their_error_texts(pima, pscale):
    """nuts_warmup and nuts_warmup_dense share one body: every refusal of an argument is worded as each of them worded it, the function's
    own name included, and is raised before any device access (the test double has no warm-up entry point)."""
    import logreg_amd as la
    import twin
    from logreg_amd import _lib
    X, y = pima
    twin.install()
    try:
        model = la.LogReg(X, y, pscale, dtype="float64")
        init = np.zeros((6, 8))
        fused = " needs a fused kernel: lpost and glp must be the closures of one LogReg (the generic NumPy NUTS has no warm-up)"
        shared = [(dict(num_warmup=0), "num_warmup must be >= 1, got 0"), (dict(max_depth=0), f"max_depth must be in 1..{_lib.NUTS_MAX_DEPTH}, got 0"),
                  (dict(target_accept=1), "target_accept must be in (0, 1), got 1"), (dict(eps=0), "eps must be finite and > 0, got 0"),
                  (dict(init=np.zeros((6, 7))), "init must be [p] or [C,p] with p=8; got (6, 7)")]
        own = {"nuts_warmup": [(dict(dmm=[1.0] * 7 + [np.nan]), "dmm must be finite and > 0"), (dict(dmm=np.inf), "dmm must be finite and > 0")],
               "nuts_warmup_dense": [(dict(inv_metric=np.ones((8, 7))), "inv_metric must be a square matrix [p, p] with p=8; got (8, 7)"),
                                     (dict(inv_metric=np.full((8, 8), np.nan)), "inv_metric must be finite")]}
        for name, cases_of in own.items():
            warm = getattr(la, name)
            for glp in (lambda b: -b, model.lpost):
                with pytest.raises(ValueError) as e:
                    warm(model.lpost, glp, init, 10)
                assert str(e.value) == name + fused
            for bad, text in shared + cases_of:
                kw = dict(init=init, num_warmup=10)
                kw.update(bad)
                with pytest.raises(ValueError) as e:
                    warm(model.lpost, model.glp, **kw)
                assert str(e.value) == text, (name, bad)
        model.close()
    finally:
        twin.uninstall()


def test_host_side_of_the_warmup_under_asan_and_ubsan():
    """tests/host/adapt_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's instantiation
    objects by tests/host_build.py."""
    last = host_build.last_line(host_build.run(host_build.harness("adapt_harness.cpp")))
    assert last.startswith("adapt harness:"), last
    assert int(last.split(":")[1].split("kernel launches")[0]) > 1000, last
