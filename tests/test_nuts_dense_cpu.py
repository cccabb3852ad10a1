"""NUTS under a dense metric (include/logreg_hip_dense.h) -- everything that can be checked without a GPU: the library's factorisation
against NumPy and its refusals, the ABI tables, the build gates with the sixteen new kernels in both builds, the planner's LDS
arithmetic and the host side of the run and of the warm-up handle (tests/host/dense_harness.cpp, a stand-alone program under
AddressSanitizer and UBSan), the Python face above the kernel, and the two independent references of tests/nuts_dense_reference.py
against each other: that comparison fixes the tolerances of tests/test_gpu_nuts_dense.py and is re-measured here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import host_build
import nuts_dense_reference as dr
import nuts_reference as nr

WANT = ["lr_dense_adapt_create", "lr_dense_adapt_destroy", "lr_dense_adapt_result", "lr_dense_adapt_run", "lr_dense_adapt_trace", "lr_dense_factor",
        "lr_run_nuts_dense"]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def _factor(L, sigma):
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    p = sigma.shape[0]
    s, R, A = np.full(p, np.nan), np.full((p, p), np.nan), np.full((p, p), np.nan)
    rc = L.lr_dense_factor(p, sigma.ctypes.data, s.ctypes.data, R.ctypes.data, A.ctypes.data)
    return rc, s, R, A


@pytest.mark.parametrize("p", [1, 3, 8, 17, 32])
def test_factorisation_against_numpy(p):
    """s, R and A = L^-T of random symmetric positive definite matrices against numpy.linalg.  The bound is the conditioning of the
    problem, not a measurement: a backward-stable Cholesky factor and triangular inverse are accurate to a small multiple of
    p * cond(R) * 2^-53, and the matrices are built with cond(R) <= 100."""
    from logreg_amd import _lib
    L = _lib.load_dense()  # (host code: needs no device)
    rng = np.random.default_rng(40 + p)
    for rep in range(5):
        R0 = dr.random_correlation(p, rng)
        D = rng.uniform(0.3, 3.0, p) * 10.0 ** rng.integers(-3, 4)
        sigma = R0 * np.outer(D, D)
        rc, s, R, A = _factor(L, sigma)
        assert rc == 0
        s_np, R_np, L_np, A_np, C_np = dr.factors(sigma)
        tol = 64 * p * 100 * 2.0 ** -53
        np.testing.assert_allclose(s, s_np, rtol=4 * 2.0 ** -53)
        np.testing.assert_allclose(R, R_np, rtol=0, atol=8 * 2.0 ** -53)
        assert np.array_equal(np.diag(R), np.ones(p)) and np.array_equal(R, R.T)
        assert np.max(np.abs(A - A_np)) <= tol * np.max(np.abs(A_np))
        assert np.array_equal(A, np.triu(A))
        B = A / s[:, None]  # p = B z has covariance B B^T = Sigma^-1
        assert np.max(np.abs(B @ B.T @ sigma - np.eye(p))) <= tol * p
        upper_nan = sigma.copy()
        upper_nan[np.triu_indices(p, 1)] = np.nan  # only the lower triangle is read
        rc2, s2, R2, A2 = _factor(L, upper_nan)
        assert rc2 == 0 and np.array_equal(A2, A) and np.array_equal(s2, s) and np.array_equal(R2, R)


def test_factorisation_refuses_what_is_not_a_metric():
    from logreg_amd import _lib
    import logreg_amd as la
    L = _lib.load_dense()
    ok = np.array([[4.0, 1.0, 0.5], [1.0, 9.0, -2.0], [0.5, -2.0, 1.0]])
    assert _factor(L, ok)[0] == 0
    cases = []
    for bad in (np.nan, np.inf, -np.inf):
        m = ok.copy()
        m[2, 0] = bad
        cases.append((m, "not finite"))
    m = ok.copy()
    m[1, 1] = 0.0
    cases.append((m, "must be > 0"))
    m = ok.copy()
    m[0, 0] = -4.0
    cases.append((m, "must be > 0"))
    cases.append((np.array([[1.0, 2.0], [2.0, 1.0]]), "not positive definite"))  # indefinite
    # rank-deficient: two copies of one coordinate, with a variance whose square root is exact (the correlation is then exactly 1 and
    # the second pivot exactly 0; after rounding, a rank-deficient matrix in general position is a barely definite or indefinite one)
    cases.append((np.array([[4.0, 4.0], [4.0, 4.0]]), "not positive definite"))
    cases.append((np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]]), "not positive definite"))
    for m, word in cases:
        rc, s, R, A = _factor(L, m)
        assert rc == -1 and word in L.lr_last_error().decode(), (m, L.lr_last_error())
        assert np.all(np.isnan(A))  # nothing written
        with pytest.raises(la.LogregHipError, match=word):
            la.nutsKernel(lambda b: 0.0, lambda b: b, 0.1, inv_metric=m)
    assert L.lr_dense_factor(0, ok.ctypes.data, None, None, None) == -1 and L.lr_dense_factor(33, ok.ctypes.data, None, None, None) == -1
    assert L.lr_dense_factor(3, None, None, None, None) == -1
    with pytest.raises(ValueError, match="square"):
        la.nutsKernel(lambda b: 0.0, lambda b: b, 0.1, inv_metric=np.ones(3))


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_dense.h") == WANT == sorted(_lib.DENSE_SYMBOLS)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.ADAPT_SYMBOLS):
        assert not set(WANT) & set(other)
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_dense_\w+|lr_run_nuts_dense)\b", exported))) == WANT, path
    assert ctypes.sizeof(_lib.AdaptOpts) == 72
    assert _lib.load_dense() is _lib.load()  # binds on first use
    src = build._sources()
    for f in (os.path.join(build.INCLUDE, "logreg_hip_dense.h"), os.path.join(build.CSRC, "lr_nuts_dense.h"), os.path.join(build.CSRC, "lr_dense.h"),
              os.path.join(build.CSRC, "lr_dense_adapt.h")):
        assert f in src, f


def test_still_13_units_and_the_dense_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        rows = b.kernel_resources(alt=alt)
        dense = [r for r in rows if "k_nuts_dense<" in r["name"]]
        assert len(dense) == 16 and not any("k_nuts<" in r["name"] for r in dense)
        diag = {re.search(r"k_nuts<(\w+), (\d+), 1, 0, (\w+)>", r["name"]).groups(): r for r in rows if "k_nuts<" in r["name"]}
        assert len(diag) == 16
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32):
                for tuned in ("false", "true"):
                    mine = [r for r in dense if f"k_nuts_dense<{dt}, {P}, 1, 0, {tuned}>" in r["name"]]
                    assert len(mine) == 1, (alt, dt, P, tuned)
                    assert mine[0]["unit"] == diag[(dt, str(P), tuned)]["unit"]  # instantiated in the existing units
                    assert mine[0]["lds"] == diag[(dt, str(P), tuned)]["lds"]    # planned as the diagonal kernel + the matrices: the same static LDS
        moments = [r for r in rows if "k_dense_comoment" in r["name"]]
        assert len(moments) == 12 and {r["unit"] for r in moments} == {"lr_api"} and all(r["lds"] <= 4096 for r in moments)
        assert not any("k_adapt_" in r["name"] for r in dense + moments)
        new = dense + moments
        assert all(r["scratch"] == 0 for r in new), [(r["name"], r["scratch"]) for r in new if r["scratch"]]
        assert all(r["vgprs"] <= 512 for r in new)
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


def test_host_side_under_asan_and_ubsan():
    """tests/host/dense_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's
    instantiation objects by tests/host_build.py: the factorisation, lr_run_nuts_dense from host
    and device memory with the per-stream factor image, the planner's LDS arithmetic and refusal message (a float64 p = 20 model of 300
    rows: 81 600 bytes of rows + 81 920 of checkpoints at max_depth 10 fit the 163 840-byte budget, 16 384 bytes of matrices more do
    not), every refusal ahead of any device access, failing allocations, and the warm-up handle across its window ends."""
    last = host_build.last_line(host_build.run(host_build.harness("dense_harness.cpp")))
    assert last.startswith("dense harness:"), last
    assert int(last.split(":")[1].split("kernel launches")[0]) > 1000, last


def test_python_face_above_the_kernel(pima, pscale):
    """nutsKernel(inv_metric=) on the CPU test double's model (no dense entry point there: nothing is launched): the kernel object, the
    checkpoint fingerprint, the new functions' signatures, and the generic NumPy NUTS under a dense metric on a correlated Gaussian."""
    import logreg_amd as la
    from logreg_amd import covariance
    params = inspect.signature(la.nutsKernel).parameters
    assert list(params) == ["lpi", "glpi", "eps", "dmm", "max_depth", "inv_metric"]
    assert params["inv_metric"].kind is inspect.Parameter.KEYWORD_ONLY and params["inv_metric"].default is None
    wp = inspect.signature(la.nuts_warmup_dense).parameters
    assert list(wp) == ["lpost", "glp", "init", "num_warmup", "target_accept", "eps", "inv_metric", "max_depth", "adapt_metric", "seed", "chain_offset", "keep"]
    with pytest.raises(ValueError, match="needs a fused kernel"):
        la.nuts_warmup_dense(lambda b: -0.5 * np.sum(b * b), lambda b: -b, np.zeros(3), 10)
    import twin
    X, y = pima
    twin.install()
    try:
        model = la.LogReg(X, y, pscale, dtype="float64")
        sig = np.diag(np.arange(1.0, 9.0)) + 0.1
        k = la.nutsKernel(model.lpost, model.glp, 0.01, max_depth=7, inv_metric=sig)
        assert isinstance(k, la.FusedKernel) and k.kind == "nuts" and "dmm" not in k.params and np.array_equal(k.params["inv_metric"], sig)
        assert k.params["inv_metric"] is not sig  # a copy: the caller's matrix may change afterwards
        kd = la.nutsKernel(model.lpost, model.glp, 0.01, 2.0, 7)
        assert "inv_metric" not in kd.params  # the diagonal kernel and its checkpoints are what they were
        with pytest.raises(ValueError, match="p=8"):
            la.nutsKernel(model.lpost, model.glp, 0.01, inv_metric=np.eye(7))
        for bad in (dict(num_warmup=0), dict(max_depth=11), dict(target_accept=1.0), dict(eps=0.0), dict(inv_metric=np.eye(7)), dict(inv_metric=np.full((8, 8), np.nan)),
                    dict(init=np.zeros((6, 7)))):
            kw = dict(init=np.zeros((6, 8)), num_warmup=10)
            kw.update(bad)
            with pytest.raises(ValueError):
                la.nuts_warmup_dense(model.lpost, model.glp, **kw)
        model.close()
    finally:
        twin.uninstall()
    # covariance.dense_metric: the warm-up's regularisation of a result's covariance; metric() keeps its two keys
    cov = np.array([[2.0, 0.3], [0.3, 1.0]])
    res = {"cov": cov, "nobs": 95}
    np.testing.assert_allclose(covariance.dense_metric(res), 0.95 * cov + 1e-3 * 0.05 * np.eye(2), rtol=1e-15)
    assert set(covariance.metric(res)) == {"dmm", "pre"}
    with pytest.raises(ValueError):
        covariance.dense_metric({"cov": np.array([[1.0, np.nan], [np.nan, 1.0]]), "nobs": 10})
    # the generic NumPy NUTS: a strongly correlated Gaussian sampled under its own covariance as the metric
    S = np.array([[1.0, 0.95, 0.0], [0.95, 1.0, 0.0], [0.0, 0.0, 25.0]])
    Si = np.linalg.inv(S)
    kern = la.nutsKernel(lambda q: -0.5 * q @ Si @ q, lambda q: -Si @ q, 0.7, max_depth=6, inv_metric=S)
    np.random.seed(4)
    x, xs = np.zeros(3), []
    for _ in range(1500):
        x = kern(x)
        xs.append(x)
    emp = np.cov(np.array(xs).T)
    assert np.max(np.abs(emp - S) / np.sqrt(np.outer(np.diag(S), np.diag(S)))) < 0.2, emp


def test_the_two_references_agree_and_fix_the_gpu_tolerances():
    """(a) the existing unit-metric reference on the whitened problem against (b) the direct plain-space restatement, over
    dr.DENSE_CASES x dr.METRICS: signed depth, leaf count and flags equal wherever both margins reach 1e-9 (at most 1 transition in
    1000 below it); the largest relative deviation of a state or acceptance statistic, times 10, is dr.DENSE_F64_TOL.  The cases must
    themselves meet the conditions the GPU test asks of them: depth >= 7 at least 10 times per padded width, at least 20 each of
    divergence, subtree and tree stops, every width and chain count of the shape set."""
    m = dr.measure_f64()
    print(f"(a) vs (b), float64: {m['n']} transitions, {m['skipped']} skipped, largest relative deviation {m['worst']:.4g}; DENSE_F64_TOL = {dr.DENSE_F64_TOL:g};",
          dict(m["reasons"]), "depth >= 7 per padded width:", dict(m["deep"]))
    assert not m["mismatches"], "\n".join(m["mismatches"][:20])
    assert m["skipped"] <= m["n"] / 1000
    assert 10 * m["worst"] <= dr.DENSE_F64_TOL <= 100 * m["worst"]  # the constant is the measurement, neither smaller nor padded
    assert all(m["deep"][P] >= 10 for P in (4, 8, 16, 32)), dict(m["deep"])
    for reason in (nr.DIVERGENCE, nr.SUBTREE, nr.TREE):
        assert m["reasons"][reason] >= 20, dict(m["reasons"])
    assert {c.p for c in dr.DENSE_CASES} == {3, 4, 5, 8, 9, 16, 17, 31, 32} and {c.C for c in dr.DENSE_CASES} == {1, 3, 65, 257}
    assert all(c.max_depth == 10 and c.chain_offset > 0 and c.iter_offset > 0 and 20 <= c.n <= 60 for c in dr.DENSE_CASES)
    for case in dr.DENSE_CASES:
        sig = dr.case_sigma(case, "dense")
        d = np.sqrt(np.diag(sig))
        assert np.linalg.cond(sig / np.outer(d, d)) <= 100 and d.min() >= 0.3 and d.max() <= 3.0
        assert np.array_equal(dr.case_sigma(case, "unit"), np.eye(case.p)) and np.count_nonzero(dr.case_sigma(case, "diag")) == case.p


def test_float32_mode_of_the_reference_fixes_the_float32_pair():
    """(b) in NumPy float32 against (b) in float64 on dr.F32_CASES x dr.METRICS, as nuts_reference.measure_float32_mode measures the
    diagonal pair: dr.DENSE_F32_TAU is 8 x the largest float64 margin at which the two modes disagreed and dr.DENSE_F32_STATE_TOL 8 x
    their largest relative deviation where they agreed, both from the larger run recorded in profiles/r19_nuts_dense.txt; this run must
    not exceed either, and at most 10 % of its margins may fall below the threshold."""
    m = dr.measure_f32()
    share = float(np.mean(m["margins"] < dr.DENSE_F32_TAU))
    print(f"(b) float32 vs float64: {m['n']} transitions, {m['disagree']} disagree (largest margin {m['tau']:.4g}), largest relative deviation {m['dev']:.4g}; "
          f"DENSE_F32_TAU = {dr.DENSE_F32_TAU:g}, DENSE_F32_STATE_TOL = {dr.DENSE_F32_STATE_TOL:g}, share of margins below the threshold {share:.4f}")
    assert 8 * m["tau"] <= dr.DENSE_F32_TAU
    assert 8 * m["dev"] <= dr.DENSE_F32_STATE_TOL
    assert share <= 0.10
