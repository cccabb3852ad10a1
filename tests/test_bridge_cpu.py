"""Bridge sampling (include/logreg_hip_bridge.h, logreg_amd/bridge.py) -- everything that can be checked without a GPU: the reference
against two-dimensional quadrature and on hand-made terms, the float32 tolerance of the GPU tests, the ABI tables and the build gates with
the new kernels in both libraries, the Python face on the CPU double (tests/twin_bridge.py), and the host harness under the sanitizers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import bridge_reference as br

WANT = ["lr_bridge_accumulate", "lr_bridge_create", "lr_bridge_destroy", "lr_bridge_proposal", "lr_bridge_reset", "lr_bridge_result", "lr_bridge_solve",
        "lr_bridge_terms"]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def _posterior_draws(X, y, ps, N, rng):
    """N independent posterior draws by sampling-importance-resampling from 2 x 10^5 draws of a widened Laplace approximation"""
    b, C = br.newton_mode(X, y, ps)
    cov = 2.25 * C
    th = b + rng.standard_normal((200000, 2)) @ np.linalg.cholesky(cov).T
    lw = br.lpost64(X, y, ps, th) - br.log_g(th, b, cov)
    w = np.exp(lw - lw.max())
    return th[rng.choice(th.shape[0], N, p=w / w.sum())]


def test_reference_against_quadrature_on_the_30_by_2_model():
    """|logml - quadrature| <= 5 se for five seeds of 4000 + 4000 draws (the proposal fitted to the first half of the posterior draws,
    the terms from the second half)."""
    X, y, ps = br.small_model(0)
    truth = br.quadrature_logml(X, y, ps, step=0.01)
    assert abs(truth - br.quadrature_logml(X, y, ps, step=0.02)) < 1e-9  # the grid has converged
    for seed in range(5):
        post = _posterior_draws(X, y, ps, 8000, np.random.default_rng(seed))
        mu, cov = post[:4000].mean(axis=0), np.cov(post[:4000].T)
        l1 = br.terms(X, y, ps, post[4000:], mu, cov)
        l2 = br.terms(X, y, ps, br.proposal_draws(seed, 4000, mu, cov), mu, cov)
        r = br.solve(l1, l2)
        z = (r["logml"] - truth) / r["se"]
        print(f"[bridge] reference, seed {seed}: quadrature {truth:.5f}, bridge {r['logml']:.5f} +- {r['se']:.1e}, {r['iterations']} iterations, z = {z:+.2f}")
        assert r["converged"] and r["iterations"] <= 6 and r["se"] < 0.01 and abs(z) <= 5.0


def test_reference_se_is_the_empirical_spread_at_unequal_sizes_and_reduced_n_eff():
    """The standard error against the spread of 120 replications on the 30 x 2 model, exact independent posterior draws by rejection
    from a widened Laplace approximation, where s1 != s2: N1 = 500 against N2 = 8000, the reverse, and draws repeated 2 and 4 times with
    n_eff = the number of distinct ones (what autocorrelation does to a chain).  The empirical root-mean-square error of 120 replications
    has a relative standard deviation of 1 / sqrt(2 x 119) = 6.5 %: the mean se must lie within a factor 1.3 (four of those) of it.  The
    two quotients of the error exchanged between the proposal and the posterior terms -- equal to these at s1 = s2 alone -- overstate it
    by factors of 1.3 to 4.6 on these cases, which the last assertion records."""
    X, y, ps = br.small_model(0)
    truth = br.quadrature_logml(X, y, ps)
    b, C = br.newton_mode(X, y, ps)
    cov = 2.25 * C
    Lc = np.linalg.cholesky(cov)
    th = b + np.random.default_rng(0).standard_normal((400000, 2)) @ Lc.T
    top = np.max(br.lpost64(X, y, ps, th) - br.log_g(th, b, cov)) + 0.05  # the envelope of the rejection sampler

    def posterior(N, rng):
        out, got = [], 0
        while got < N:
            th = b + rng.standard_normal((4 * N + 1000, 2)) @ Lc.T
            keep = th[np.log(rng.random(th.shape[0])) < br.lpost64(X, y, ps, th) - br.log_g(th, b, cov) - top]
            out.append(keep)
            got += keep.shape[0]
        return np.concatenate(out)[:N]

    def exchanged_se(l1, l2, lr, neff):
        s1, s2 = neff / (neff + l2.size), l2.size / (neff + l2.size)
        f1, f2 = 1.0 / (s1 * np.exp(l2 - lr) + s2), 1.0 / (s1 + s2 * np.exp(lr - l1))
        return np.sqrt(np.var(f1, ddof=1) / (np.mean(f1) ** 2 * l2.size) + np.var(f2, ddof=1) / (np.mean(f2) ** 2 * neff))
    worst = 0.0
    for N1, N2, rep in ((500, 8000, 1), (8000, 500, 1), (2000, 4000, 2), (1000, 4000, 4)):
        est, ses, other = [], [], []
        for k in range(120):
            rng = np.random.default_rng(1000 + k)
            fit = posterior(2000, rng)
            mu, S = fit.mean(axis=0), np.cov(fit.T)
            l1 = br.terms(X, y, ps, np.repeat(posterior(N1, rng), rep, axis=0), mu, S)
            l2 = br.terms(X, y, ps, br.proposal_draws(k, N2, mu, S), mu, S)
            r = br.solve(l1, l2, n_eff=float(N1))
            est.append(r["logml"])
            ses.append(r["se"])
            other.append(exchanged_se(l1, l2, r["logml"], float(N1)))
        rmse = float(np.sqrt(np.mean((np.array(est) - truth) ** 2)))
        print(f"[bridge] N1 = {N1} x {rep}, N2 = {N2}: rmse of 120 replications {rmse:.5f}, mean se {np.mean(ses):.5f} (ratio {np.mean(ses) / rmse:.3f}); "
              f"the quotients exchanged: {np.mean(other):.5f} (ratio {np.mean(other) / rmse:.3f})")
        assert 1 / 1.3 <= np.mean(ses) / rmse <= 1.3, (N1, N2, rep, rmse, np.mean(ses))
        worst = max(worst, float(np.mean(other) / rmse))
    assert worst > 3.0


def test_reference_on_hand_made_terms():
    for c in (-3.3, 0.0, 712.5, -1e4):
        for n1, n2, neff in ((10, 7, None), (1, 1, None), (400, 9, 30.0)):
            r = br.solve(np.full(n1, c), np.full(n2, c), n_eff=neff)
            assert r["logml"] == c and r["iterations"] == 1 and r["converged"] and r["se"] == 0.0, (c, n1, n2, r)
    # g = the normalised density itself: every term is log Z, whatever the draws
    r = br.solve(np.full(50, 1.25), np.full(60, 1.25), maxit=0)
    assert r["logml"] == 1.25 and r["iterations"] == 0 and not r["converged"]
    # two unnormalised Gaussians, q1 = exp(-x^2 / 2) against g = N(0, 1.5^2): log Z = log sqrt(2 pi)
    rng = np.random.default_rng(5)
    x1, x2 = rng.standard_normal(20000), 1.5 * rng.standard_normal(20000)
    lg = lambda x: -0.5 * (x / 1.5) ** 2 - np.log(1.5) - 0.5 * np.log(2 * np.pi)  # noqa: E731
    r = br.solve(-0.5 * x1 ** 2 - lg(x1), -0.5 * x2 ** 2 - lg(x2))
    assert abs(r["logml"] - 0.5 * np.log(2 * np.pi)) <= 5 * r["se"] and r["se"] < 0.01
    bad = br.solve(np.array([0.0, np.nan]), np.array([0.0, -np.inf, 1.0]))
    assert np.isnan(bad["logml"]) and np.isnan(bad["se"]) and bad["n_nonfinite"] == 2
    d = np.abs(np.diff(br.solve(-0.5 * x1 ** 2 - lg(x1), -0.5 * x2 ** 2 - lg(x2), tol=1e-14)["trace"]))
    assert np.all(d[1:][d[:-1] > 1e-13] / d[:-1][d[:-1] > 1e-13] < 0.5)  # a contraction


def test_reference_proposal_draws_and_gaussian():
    from scipy.stats import multivariate_normal
    c = br.term_case(8, 5, seed=2, S=50)
    rng = np.random.default_rng(1)
    A = rng.standard_normal((8, 8))
    S, m, B = A @ A.T + 8 * np.eye(8), rng.standard_normal(8), 3 * rng.standard_normal((50, 8))  # (well conditioned: scipy goes through an eigendecomposition)
    assert np.max(np.abs(br.log_g(B, m, S) - multivariate_normal(m, S).logpdf(B))) < 1e-11
    d = br.proposal_draws(3, 4000, c["mu"], c["cov"])
    assert d[:1000].tobytes() == br.proposal_draws(3, 1000, c["mu"], c["cov"]).tobytes() and not np.array_equal(d[:10], br.proposal_draws(4, 10, c["mu"], c["cov"]))
    z = br.proposal_normals(3, np.arange(4000), 8)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    assert np.array_equal(br.proposal_normals(3, [2 ** 33 + 5], 8), br.proposal_normals(3, [2 ** 33 + 5], 8)) and not np.array_equal(
        br.proposal_normals(3, [2 ** 33 + 5], 8), br.proposal_normals(3, [5], 8))  # the high word of j counts


def test_float32_tolerances_of_the_gpu_tests_are_the_measured_ones():
    """F32_UNITS[n] is 8 x the largest deviation of the reference's float32 mode from its float64 mode over the GPU test's own cases
    (within a tenth, rounded up), in units of one float32 ulp of every row's magnitudes."""
    worst = {n: 0.0 for n in br.ROWS}
    for p in br.WIDTHS:
        for n in br.ROWS:
            c = br.rounded(br.gpu_term_case(p, n), np.float32)
            a, b = (br.terms(c["X"], c["y"], c["pscale"], c["B"], c["mu"], c["cov"], mode) for mode in ("float32", "float64"))
            worst[n] = max(worst[n], float(np.max(np.abs(a - b) / br.term_unit32(c["X"], c["B"]))))
    c = br.rounded(br.saturated_case(), np.float32)
    a, b = (br.terms(c["X"], c["y"], c["pscale"], c["B"], c["mu"], c["cov"], mode) for mode in ("float32", "float64"))
    worst["saturated"] = float(np.max(np.abs(a - b) / br.term_unit32(c["X"], c["B"])))
    print("[bridge] float32 mode against float64 mode, units:", {k: round(v, 4) for k, v in worst.items()})
    for k, v in worst.items():
        assert 8 * v <= br.F32_UNITS[k] <= 8 * v * 1.1 + 0.05, (k, v, br.F32_UNITS[k])


def test_float64_bound_is_small_against_the_terms():
    """The bound the GPU test holds float64 terms to is a few hundred ulp of the term at most, and the reference's float64 mode with the
    rows summed in another order stays far inside it."""
    for p, n in ((3, 63), (33, 257), (128, 601)):
        c = br.gpu_term_case(p, n)
        B = c["B"][:200]
        t = br.terms(c["X"], c["y"], c["pscale"], B, c["mu"], c["cov"])
        bound = br.term_bound64(c["X"], c["pscale"], B, c["mu"], c["cov"])
        perm = np.random.default_rng(0).permutation(n)
        t2 = br.terms(c["X"][perm], c["y"][perm], c["pscale"], B, c["mu"], c["cov"])
        assert np.all(bound < 1e-9 * np.abs(t) + 1e-9) and np.all(np.abs(t - t2) <= 0.25 * bound)


# ---- ABI and build ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_table_matches_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_bridge.h") == WANT == sorted(_lib.BRIDGE_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.PG_SYMBOLS):
        assert not set(WANT) & set(other)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38  # logreg_hip.h's set stays as pinned
    hdr = open(os.path.join(REPO, "include", "logreg_hip_bridge.h")).read()
    assert int(re.search(r"#define LR_BRIDGE_ROWS (\d+)", hdr).group(1)) == _lib.BRIDGE_ROWS == 12
    assert int(re.search(r"#define LR_BRIDGE_MAX_DRAWS (\d+)", hdr).group(1)) == _lib.BRIDGE_MAX_DRAWS >= 1 << 20
    assert int(re.search(r"#define LR_BRIDGE_TAG (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == _lib.BRIDGE_TAG == br.BRIDGE_TAG
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_bridge_\w+)", exported))) == WANT, path
    assert _lib.load_bridge() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_bridge.h") in src and os.path.join(build.CSRC, "lr_bridge.h") in src


def test_still_13_units_and_the_bridge_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_bridge_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32, 64, 128):
                for k in ("fill", "gauss", "propose"):
                    assert sum(f"k_bridge_{k}<{dt}, {P}>" in r["name"] for r in mine) == 1, (alt, k, dt, P)
        assert sum("k_bridge_iterate" in r["name"] for r in mine) == 1 and sum("k_bridge_finish" in r["name"] for r in mine) == 1
        assert len(mine) == 38
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert all(r["lds"] <= 64 * 1024 for r in mine)
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


# ---- the Python face ---------------------------------------------------------------------------------------------------------------------------
def test_no_gpu_means_loud_failure_not_fallback():
    import logreg_amd as la
    if la.device_count() > 0:  # with a device the same calls get as far as their argument checks
        with pytest.raises(TypeError):
            la.Bridge(None, np.zeros(2), np.eye(2), 10)
        return
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.Bridge(None, np.zeros(2), np.eye(2), 10)
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.bridge_sampling(None, np.zeros((4, 2)), np.zeros(2), np.eye(2))
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.bridge_from_terms(np.zeros(3), np.zeros(3))


def test_bridge_is_keyword_only_between_loo_and_covariance():
    import logreg_amd as la
    params = inspect.signature(la.mcmc).parameters
    assert params["bridge"].kind is inspect.Parameter.KEYWORD_ONLY and params["bridge"].default is None
    names = list(params)
    assert names[names.index("loo") + 1] == "bridge" and names[-3:] == ["covariance", "marginals", "predictive"] and names[names.index("bridge") + 1] == "covariance"
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, bridge=object())


def test_pure_numpy_helpers():
    import logreg_amd as la
    a = la.bridge_from_table([-10.0, 0.03, 4, 1, 100, 200, 50.0, 0, -12, -8, -13, -7])
    b = la.bridge_from_table([-12.5, 0.04, 3, 1, 100, 200, 100.0, 0, -12, -8, -13, -7])
    assert a["converged"] and a["iterations"] == 4 and a["n_draws"] == 100 and a["n_proposal"] == 200 and a["n_eff"] == 50.0 and a["l2_max"] == -7
    c = la.bridge_compare(a, b)
    assert c["log_bf"] == 2.5 and abs(c["se"] - 0.05) < 1e-15 and abs(c["prob_a"] - 1 / (1 + np.exp(-2.5))) < 1e-15
    assert la.bridge_compare(b, a)["log_bf"] == -2.5
    with pytest.raises(ValueError):
        la.bridge_from_table(np.zeros(11))
    mean, cov = la.bridge_proposal({"mean": [1.0, 2.0], "cov": [[2.0, 0.5], [0.5000001, 1.0]]})
    assert np.array_equal(mean, [1.0, 2.0]) and np.array_equal(cov, cov.T)
    mean, cov = la.bridge_proposal((np.zeros(3), np.eye(3)))
    assert cov.shape == (3, 3)
    for bad in ((np.zeros(3), np.eye(2)), {"mean": [np.nan], "cov": [[1.0]]}, 5):
        with pytest.raises((ValueError, TypeError)):
            la.bridge_proposal(bad)


def test_python_face_on_the_cpu_double(pima, pscale):
    """tests/twin_bridge.py: refusals of shapes, types and matrices that are not covariances; terms, proposal draws and the result
    against the reference; mcmc(..., bridge=acc) equals feeding the kept draws by hand; reset keeps the proposal terms."""
    import logreg_amd as la
    from logreg_amd import _lib
    import twin
    import twin_bridge
    X, y = pima
    L0 = twin.install()  # a library without the entry points
    try:
        model = la.LogReg(X, y, pscale, dtype="float64")
        assert not hasattr(L0, "lr_bridge_create")
        with pytest.raises(la.LogregHipError, match="no bridge-sampling entry points"):
            la.Bridge(model, np.zeros(8), np.eye(8), 10)
        with pytest.raises(la.LogregHipError, match="no bridge-sampling entry points"):
            la.bridge_from_terms(np.zeros(3), np.zeros(3))
        model.close()
    finally:
        twin.uninstall()
    L = twin_bridge.install()
    try:
        assert _lib.load() is L and _lib.load_bridge() is L
        model = la.LogReg(X, y, pscale, dtype="float64")
        b, C = br.newton_mode(X, y, pscale)
        with pytest.raises(TypeError, match="LogReg"):
            la.Bridge("model", b, C, 10)
        for bad in (10.5, True):
            with pytest.raises(TypeError, match="integer"):
                la.Bridge(model, b, C, bad)
        for bad in (0, -3):
            with pytest.raises(ValueError, match="positive"):
                la.Bridge(model, b, C, bad)
            with pytest.raises(ValueError, match="positive"):
                la.Bridge(model, b, C, 10, n_proposal=bad)
        with pytest.raises(ValueError, match="beyond"):
            la.Bridge(model, b, C, (1 << 20) + 1)
        with pytest.raises(ValueError, match=r"\[p, p\]"):
            la.Bridge(model, b[:7], C, 10)
        with pytest.raises(ValueError, match=r"\[p, p\]"):
            la.Bridge(model, b, C[:7], 10)
        with pytest.raises(ValueError, match="seed"):
            la.Bridge(model, b, C, 10, seed=-1)
        for k, v in ((0, np.nan), (3, np.inf)):
            bb = b.copy()
            bb[k] = v
            with pytest.raises(ValueError, match="finite"):
                la.Bridge(model, bb, C, 10)
        Cn = C.copy()
        Cn[2, 1] = Cn[1, 2] = np.nan
        with pytest.raises(ValueError, match="finite and symmetric"):
            la.Bridge(model, b, Cn, 10)
        Ca = C.copy()
        Ca[2, 1] *= 1.5
        with pytest.raises(ValueError, match="symmetric"):
            la.Bridge(model, b, Ca, 10)
        with pytest.raises(ValueError, match="not a covariance matrix.*positive definite"):
            la.Bridge(model, b, C - 2 * np.max(np.diag(C)) * np.eye(8), 10)
        with pytest.raises(ValueError, match="not a covariance matrix.*positive definite"):
            la.Bridge(model, b, np.zeros((8, 8)), 10)
        with pytest.raises(ValueError, match=r"\[S, p\]"):
            la.bridge_sampling(model, np.zeros(8), b, C)

        rng = np.random.default_rng(0)
        draws = b + rng.standard_normal((600, 8)) @ np.linalg.cholesky(C).T
        acc = la.Bridge(model, b, 1.3 * C, max_draws=700, n_proposal=500, seed=9)
        assert "n_draws=0" in repr(acc) and np.isnan(acc.result()["logml"]) and acc.result()["n_proposal"] == 500
        acc.update(draws[:250]).update(draws[250:].reshape(7, 50, 8))
        l1, l2 = acc.terms()
        prop = acc.proposal_draws()
        assert np.max(np.abs(prop - br.proposal_draws(9, 500, b, 1.3 * C))) < 1e-12
        assert np.max(np.abs(l1 - br.terms(X, y, pscale, draws, b, 1.3 * C))) < 1e-9 and np.max(np.abs(l2 - br.terms(X, y, pscale, prop, b, 1.3 * C))) < 1e-9
        for kw in ({}, {"n_eff": 120.0}, {"tol": 1e-4}, {"maxit": 1}):
            res, ref = acc.result(**kw), br.solve(l1, l2, **kw)
            assert abs(res["logml"] - ref["logml"]) < 1e-10 and abs(res["se"] / ref["se"] - 1) < 1e-9 and res["iterations"] == ref["iterations"]
            assert res["converged"] == ref["converged"] and res["n_eff"] == ref["n_eff"] and res["n_draws"] == 600
            assert la.bridge_from_terms(l1, l2, **kw)["table"].tobytes() == res["table"].tobytes()
        one = la.bridge_sampling(model, draws, b, 1.3 * C, n_proposal=500, seed=9)
        assert one["table"].tobytes() == acc.result()["table"].tobytes()
        for bad in (np.zeros((4, 7)), np.zeros((0, 8)), np.zeros((2, 3, 4, 8))):
            with pytest.raises(ValueError):
                acc.update(bad)
        with pytest.raises(ValueError, match="exceed max_draws"):
            acc.update(np.zeros((101, 8)))
        for kw in ({"n_eff": -1.0}, {"n_eff": np.nan}, {"tol": -1.0}, {"maxit": -1}, {"maxit": 2.5}):
            with pytest.raises(ValueError):
                acc.result(**kw)
        acc.reset()
        assert acc.n_draws == 0 and acc.terms()[1].tobytes() == l2.tobytes() and acc.terms()[0].size == 0
        bad = draws[:5].copy()
        bad[3, 2] = np.nan
        r = acc.update(bad).result()
        assert np.isnan(r["logml"]) and np.isnan(r["se"]) and r["n_nonfinite"] == 1 and np.isfinite(r["l1_min"])
        acc.reset()

        # mcmc(..., bridge=acc) equals feeding the kept draws by hand
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.tile(b, (6, 1))
        for name, wrong in (("must be a Bridge", "yes"), ("must be a Bridge", la.Autocorr(6, 8, "float64"))):
            with pytest.raises(ValueError, match=name):
                la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, bridge=wrong)
        other = la.LogReg(X, y, pscale, dtype="float32")
        foreign = la.Bridge(other, b, C, 100, n_proposal=10)
        with pytest.raises(ValueError, match="own model"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, bridge=foreign)
        small = la.Bridge(model, b, C, 11, n_proposal=10)
        with pytest.raises(ValueError, match="max_draws = 11"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, bridge=small)
        out, info = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, return_info=True, bridge=acc, chunk=7)
        assert acc.n_draws == 120 and info["bridge"]["n_draws"] == 120
        by_hand = la.Bridge(model, b, 1.3 * C, max_draws=700, n_proposal=500, seed=9).update(out)
        assert by_hand.terms()[0].tobytes() == acc.terms()[0].tobytes() and by_hand.result()["table"].tobytes() == info["bridge"]["table"].tobytes()
        acc.reset()
        summ = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, summary_only=True, bridge=acc)
        assert summ["bridge"]["table"].tobytes() == info["bridge"]["table"].tobytes()  # the same draws without a sample matrix
        plain = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4)
        assert plain.tobytes() == out.tobytes()  # the chains are those of the same call without it
        for a in (acc, by_hand, foreign, small):
            a.close()
        with pytest.raises(la.LogregHipError, match="closed"):
            acc.update(draws[:2])
        other.close()
        model.close()
    finally:
        twin_bridge.uninstall()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------
def test_host_harness_under_the_sanitizers():
    """tests/host/bridge_harness.cpp on the stub runtime, built under AddressSanitizer + UBSan by tests/host_build.py: every allocation
    of create, accumulate and solve fails in turn."""
    import host_build
    r = host_build.run(host_build.harness("bridge_harness.cpp", "asan"))
    line = host_build.last_line(r)
    print("[bridge]", line)
    assert line.startswith("bridge harness:") and line.endswith(" 0 failures")
