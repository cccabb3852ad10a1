"""The NUTS warm-up on the stepwise engine (include/logreg_hip_adapt_tall.h, logreg_amd/adapt.py nuts_warmup_stepwise) -- everything that can be
checked without a GPU: the ABI table, the build gates with the new kernels in both builds, the reference (tests/adapt_reference.py) against
a NumPy restatement of the header's workgroup order at the wide lane maps, the four mutations on a recorded device trace of a wide case,
the Python face's argument checks, and the host side (tests/host/adapt_tall_harness.cpp, a stand-alone program) under AddressSanitizer
and UBSan."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import host_build
import adapt_reference as ar
import adapt_tall_cases as cases

WANT = ["lr_tall_adapt_create", "lr_tall_adapt_run"]


def test_symbol_table_matches_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    txt = open(os.path.join(REPO, "include", "logreg_hip_adapt_tall.h")).read()
    assert sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt))) == WANT == sorted(_lib.ADAPT_TALL_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.ADAPT_SYMBOLS, _lib.DENSE_SYMBOLS, _lib.PG_SYMBOLS):
        assert not set(WANT) & set(other)
    assert _lib.ADAPT_TALL_SYMBOLS["lr_tall_adapt_run"] == _lib.ADAPT_SYMBOLS["lr_adapt_run"]  # lr_adapt_run's signature
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_tall_adapt_\w+)", exported))) == WANT, path
    assert _lib.load_adapt_tall() is _lib.load() and hasattr(_lib.load().lr_adapt_result, "argtypes")  # binds the handle's readers too
    assert os.path.join(build.INCLUDE, "logreg_hip_adapt_tall.h") in build._sources()
    for p, P in ((3, 4), (8, 8), (20, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
        assert cases.padded(p) == P
    m = re.search(r"#define LR_ADAPT_TALL_WIDTH\(p\) \(\(p\) <= 32 \? LR_ADAPT_WIDTH\(p\) : \(p\) <= 64 \? 64 : 128\)", txt)
    assert m is not None


def test_still_13_units_and_the_new_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        rows = b.kernel_resources(alt=alt)
        wide = [r for r in rows if "k_tall_adapt_" in r["name"]]
        assert {r["unit"] for r in wide} == {"lr_api"} and len(wide) == 8
        for dt in ("float", "double"):
            for P in (64, 128):
                for k in ("k_tall_adapt_partial", "k_tall_adapt_update"):
                    assert sum(f"{k}<{dt}, {P}>" in r["name"] for r in wide) == 1, (alt, k, dt, P)
        tuned = [r for r in rows if "k_tall_nuts_update_tuned<" in r["name"]]
        plain = [r for r in rows if "k_tall_nuts_update<" in r["name"]]
        assert len(tuned) == 12 == len(plain) and {r["unit"] for r in tuned} == {r["unit"] for r in plain}
        new = wide + tuned + [r for r in rows if "k_adapt_" in r["name"]]
        assert all(r["scratch"] == 0 for r in new), [(r["name"], r["scratch"]) for r in new if r["scratch"]]
        assert all(r["lds"] <= 4096 for r in wide)
        key = lambda r: re.search(r"k_tall_nuts_update(?:_tuned)?<(\w+), (\d+)", r["name"]).groups()  # noqa: E731
        lds = {key(r): r["lds"] for r in tuned}
        for r in plain:  # the tuned kernel runs in the plain one's launches: the same static LDS
            assert lds[key(r)] == r["lds"]
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


@pytest.mark.parametrize("Cn", [1, 255, 257])
@pytest.mark.parametrize("p", [33, 64, 65, 128])
def test_the_reference_holds_the_headers_order_within_its_own_bounds(p, Cn):
    """Synthetic acceptance statistics and draws through adapt_reference.teacher_forced (np.longdouble, two passes) and through the header's
    arithmetic in the header's order (adapt_tall_cases.header_order: Q = 4 and 2 lane-strided sums, the tree over Q, Chan merges in
    workgroup order, then into the window): the latter lies within the former's input-derived bounds -- the bounds the GPU test uses."""
    W = 40
    rng = np.random.default_rng(1000 * p + Cn)
    astat = rng.uniform(0.0, 1.0, (W, Cn)) * (rng.uniform(size=(W, Cn)) > 0.1)
    scale = 10.0 ** rng.uniform(-3, 2, p)
    draws = (rng.standard_normal((W, Cn, p)) * scale + 5.0 * scale * rng.standard_normal(p)).astype(np.float32 if p % 2 else np.float64)
    tf = ar.teacher_forced(astat, draws, W, np.ones(p))
    ho = cases.header_order(astat, draws, W, np.ones(p))
    assert np.all(np.abs(ho["abar"] - tf["abar"]) <= tf["tol_abar"])
    assert len(ho["metric"]) == len(tf["metric"]) == 1 and ho["skipped"] == tf["skipped"]
    for (var, dmm, skipped), mt in zip(ho["metric"], tf["metric"]):
        assert np.array_equal(skipped, mt["skipped"])
        ok = ~skipped
        assert np.all(np.abs(var - mt["var"])[ok] <= mt["tol_var"][ok]), np.max((np.abs(var - mt["var"]) / mt["tol_var"])[ok])
        assert np.all(np.abs(dmm - mt["dmm"]) <= mt["tol_dmm"])
        if Cn > 1:
            assert np.any(var != mt["var"])  # (another order: not the reference's own bits, or the comparison would say nothing)
    assert np.all(np.abs(ho["dmm"] - tf["dmm"]) <= tf["metric"][-1]["tol_dmm"])


def test_each_mutation_fails_on_the_recorded_wide_trace():
    """tests/golden/adapt_tall_trace_p65_W150.json: abar_t, the step each iteration used and log_eps_bar of a float64 warm-up at p = 65 (P = 128),
    C = 65, W = 150, recorded on the MI355X.  The reference passes at the tolerance of tests/test_gpu_adapt_tall.py; with t0 = 11, kappa = 0.76,
    m off by one, or a restart that keeps Hbar it must not."""
    g = load_golden("adapt_tall_trace_p65_W150.json")
    abar, eps_dev, leb_dev = np.array(g["abar"]), np.array(g["eps"]), np.array(g["log_eps_bar"])
    init, ends = ar.schedule(len(abar))
    assert (init, ends) == (75, [100]) and len(abar) == 150

    def dev(**kw):
        d = ar.dual_averaging(abar, [e - 1 for e in ends], **kw)
        return max(np.max(np.abs(d["eps"] - eps_dev) / eps_dev), np.max(np.abs(d["log_eps_bar"] - leb_dev) / np.maximum(np.abs(leb_dev), 1.0)), abs(d["final"] - g["final"]) / g["final"])
    assert dev() <= cases.EPS_RTOL
    for name, kw in (("t0 = 11", dict(t0=11.0)), ("kappa = 0.76", dict(kappa=0.76)), ("m off by one", dict(m_offset=1)), ("restart keeps Hbar", dict(keep_hbar=True))):
        assert dev(**kw) > 1e3 * cases.EPS_RTOL, (name, dev(**kw))


def test_nuts_warmup_stepwise_is_nuts_warmup_with_the_engine_as_data(pima, pscale):
    """The stepwise warm-up is a function of its own beside `nuts_warmup`, whose parameter list tests/test_adapt_cpu.py pins (as
    `nuts_warmup_dense` is): the same parameters, one shared body, its own name in the refusals."""
    import logreg_amd as la
    from logreg_amd import adapt
    assert "nuts_warmup_stepwise" in la.__all__
    assert str(inspect.signature(la.nuts_warmup_stepwise)) == str(inspect.signature(la.nuts_warmup))
    assert "mode" not in inspect.signature(la.nuts_warmup).parameters and "mode" not in inspect.signature(la.nuts_warmup_dense).parameters
    src = inspect.getsource(adapt)
    assert src.count("def _warmup(") == 1 and src.count("_run\")(") == 1  # one body
    with pytest.raises(ValueError, match="nuts_warmup_stepwise needs a fused kernel"):
        la.nuts_warmup_stepwise(lambda b: -0.5 * np.sum(b * b), lambda b: -b, np.zeros(3), 10)
    import twin
    X, y = pima
    twin.install()
    try:
        model = la.LogReg(X, y, pscale, dtype="float64")
        with pytest.raises(ValueError, match="dmm must be finite and > 0"):
            la.nuts_warmup_stepwise(model.lpost, model.glp, np.zeros((6, 8)), 10, dmm=0.0)
        with pytest.raises(la.LogregHipError, match="no stepwise warm-up entry points"):  # a library without the new header says so
            la.nuts_warmup_stepwise(model.lpost, model.glp, np.zeros((6, 8)), 10)
        model.close()
    finally:
        twin.uninstall()


def test_host_side_of_the_stepwise_warmup_under_asan_and_ubsan():
    """tests/host/adapt_tall_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's
    instantiation objects by tests/host_build.py."""
    last = host_build.last_line(host_build.run(host_build.harness("adapt_tall_harness.cpp")))
    assert last.startswith("adapt tall harness:"), last
    assert int(last.split(":")[1].split("kernel launches")[0]) > 1000, last
