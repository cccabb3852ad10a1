"""Posterior predictive checks (include/logreg_hip_ppc.h, logreg_amd/ppc.py) -- everything that can be checked without a GPU: the
reference on hand-made cases, the undecided share of every GPU case under its cap, the CPU double against the reference, the Python
face on the double (every refusal, the mcmc keyword), the ABI tables and the build gates with the new kernels in both libraries, and the
host harness under the sanitizers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
import ppc_cases as pc
import ppc_reference as ppr

WANT = ["lr_ppc_accumulate", "lr_ppc_create", "lr_ppc_destroy", "lr_ppc_reset", "lr_ppc_result", "lr_ppc_terms"]


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def test_uniforms_are_words_of_one_block_per_four_draws():
    """u(s, i) is word s & 3 of the block of (s >> 2, i): four consecutive draws share a block, the fifth starts the next; a first
    index moves the window and nothing else."""
    import pg_reference as pg
    u = ppr.uniforms(11, 0, 9, 5)
    for s in (0, 3, 4, 8):
        for i in (0, 4):
            w = pg.philox(s >> 2, 0, i, ppr.TAG, 11, 0)
            assert u[s, i] == ((int(w[s & 3]) >> 8) + 0.5) * 2.0 ** -24
    assert np.array_equal(ppr.uniforms(11, 3, 6, 5), u[3:9]) and not np.array_equal(ppr.uniforms(12, 0, 9, 5), u)
    big = ppr.uniforms(11, (1 << 34) + 2, 3, 2)  # the high word of q enters the counter
    assert np.all((big > 0) & (big < 1)) and not np.array_equal(big, ppr.uniforms(11, 2, 3, 2))
    u32 = ppr.uniforms(11, 0, 9, 5, "float32")  # the 25-bit sum rounded to float32, to even
    assert np.array_equal(u32.astype(np.float32).astype(np.float64), u32) and np.max(np.abs(u32 - u)) == 2.0 ** -25


def test_saturated_probabilities_give_deterministic_replicates():
    """pi = 0 and pi = 1 exactly: every replicate is 0, or 1, whatever the uniform, and no pair is undecided"""
    X = np.array([[1.0, 0.0], [-1.0, 0.0], [1.0, 1.0]])
    B = np.tile([[5000.0, 0.0]], (40, 1))
    for dtype in pc.DTYPES:
        pv = ppr.pair_values(X, B, dtype)
        rep, und, _ = ppr.replicate(pv, 3)
        assert np.all(pv["pi"][:, 0] == 1.0) and np.all(pv["pi"][:, 1] == 0.0)
        assert np.all(rep[:, 0]) and not np.any(rep[:, 1]) and np.all(rep[:, 2]) and not np.any(und)
        D, bound = ppr.deviance(pv, rep)
        assert np.all(D == 0.0) and np.all(np.isfinite(bound))
        D, _ = ppr.deviance(pv, ~rep)
        assert np.all(D == 2 * 15000.0)


def test_tables_from_hand_made_terms_and_the_python_result():
    """Three groups, the last one empty: histogram sums equal the number of finite draws, p_ge + p_le - P(T = T_obs) = 1, quantiles are
    exact, a non-finite draw counts for nothing but itself."""
    import logreg_amd as la
    rep = np.array([[1, 0, 1, 1], [0, 0, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1]], dtype=bool)
    groups, n_g = np.array([0, 1, 0, 1]), np.array([2, 2, 0])
    counts = ppr.counts_of(rep, groups, 3)
    assert counts.tolist() == [[2, 1, 0], [1, 0, 0], [2, 2, 0], [0, 0, 0], [1, 1, 0]]
    dev = np.array([[10.0, 12.0], [11.0, 9.0], [10.5, 10.5], [np.nan, np.nan], [12.0, 14.0]])
    fin = np.array([1, 1, 1, 0, 1], dtype=bool)
    t = ppr.accumulate(counts, dev, rep, n_g, fin)
    assert t["hist"].tolist() == [0, 2, 2, 1, 2, 1, 4] and t["row_ones"].tolist() == [3, 1, 3, 3] and t["counts"].tolist() == [3, 1] and t["n_draws"] == 5
    assert abs(t["moments"][0] - 10.875) < 1e-15 and abs(t["moments"][1] - 2.1875) < 1e-14
    res = la.ppc_from_table(t_obs=[1, 2, 0], n_g=n_g, **t)
    assert res["n"] == 4 and res["n_nonfinite"] == 1 and res["n_draws"] == 5 and [int(h.sum()) for h in res["hist"]] == [4, 4, 4]
    assert res["mean"].tolist() == [1.5, 1.0, 0.0] and res["p_ge"].tolist() == [1.0, 0.25, 1.0] and res["p_le"].tolist() == [0.5, 1.0, 1.0]
    for g in range(3):
        assert res["p_ge"][g] + res["p_le"][g] - res["hist"][g][res["t_obs"][g]] / res["n"] == 1.0
    assert res["p_two"].tolist() == [1.0, 0.5, 1.0] and res["dev_p"] == 0.75 and res["row_freq"].tolist() == [0.75, 0.25, 0.75, 0.75]
    assert abs(res["sd"][0] - np.std([2, 1, 2, 1], ddof=1)) < 1e-15 and abs(res["dev_obs_sd"] - np.sqrt(2.1875 / 3)) < 1e-15
    assert res.quantile(0.0).tolist() == [1, 0, 0] and res.quantile(0.5).tolist() == [1, 1, 0] and res.quantile(0.75).tolist() == [2, 1, 0]
    assert res.quantile(1.0).tolist() == [2, 2, 0] and res.quantile(1.0, rate=True)[:2].tolist() == [1.0, 1.0] and np.isnan(res.quantile(0.5, rate=True)[2])
    assert res["rate_obs"][:2].tolist() == [0.5, 1.0] and res["rate_mean"][:2].tolist() == [0.75, 0.5]
    again = la.ppc_from_table(**res["tables"])
    assert again["p_two"].tolist() == res["p_two"].tolist() and again["tables"]["hist"].tobytes() == t["hist"].tobytes()
    with pytest.raises(ValueError, match="fit together"):
        la.ppc_from_table(t["hist"][:-1], t["row_ones"], t["counts"], t["moments"], [1, 2, 0], n_g, 5)
    with pytest.raises(ValueError, match="finite draws"):
        la.ppc_from_table(t["hist"], t["row_ones"], t["counts"], t["moments"], [1, 2, 0], n_g, 6)
    with pytest.raises(ValueError):
        res.quantile(1.5)
    empty = la.ppc_from_table(np.zeros(7), np.zeros(4), np.zeros(2), np.full(4, np.nan), [-1, -1, -1], n_g, 0)
    assert np.all(np.isnan(empty["p_two"])) and np.isnan(empty["dev_p"]) and np.all(np.isnan(empty.quantile(0.5))) and np.all(np.isnan(empty["row_freq"]))


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: "r%d_p%d_S%d" % c)
def test_undecided_share_of_every_gpu_case_is_under_the_cap(case, dtype):
    """At most 0.1 % of a case's pairs lie within tol_pi of their uniform, and every case has at least 4000 pairs"""
    ref = pc.reference(*case, dtype)
    pairs, und = ref["rep"].size, int(ref["undecided"].sum())
    print(f"[ppc] {case} {dtype}: {und} of {pairs} pairs undecided, replicate rate {ref['rep'].mean():.3f}")
    assert pairs >= ppr.MIN_PAIRS and und <= ppr.UNDECIDED_CAP * pairs
    assert 0.02 < ref["rep"].mean() < 0.98  # the case exercises both outcomes
    if dtype == "float64":
        assert und == 0


# ---- ABI and build ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_table_matches_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_ppc.h") == WANT == sorted(_lib.PPC_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.PG_SYMBOLS,
                  _lib.BRIDGE_SYMBOLS, _lib.RANK_SYMBOLS):
        assert not set(WANT) & set(other)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38  # logreg_hip.h's set stays as pinned
    hdr = open(os.path.join(REPO, "include", "logreg_hip_ppc.h")).read()
    assert int(re.search(r"#define LR_PPC_MAX_GROUPS (\d+)", hdr).group(1)) == _lib.PPC_MAX_GROUPS == 32
    assert int(re.search(r"#define LR_PPC_MOMENTS (\d+)", hdr).group(1)) == _lib.PPC_MOMENTS == 4
    assert int(re.search(r"#define LR_PPC_TAG (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == _lib.PPC_TAG == ppr.TAG == 0x04000000
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_ppc_\w+)", exported))) == WANT, path
    assert _lib.load_ppc() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_ppc.h") in src and os.path.join(build.CSRC, "lr_ppc.h") in src


def test_still_13_units_and_the_ppc_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_ppc_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for dt in ("float", "double"):
            assert sum(f"k_ppc_flag<{dt}>" in r["name"] for r in mine) == 1
            for P in (4, 8, 16, 32, 64, 128):
                for lab in ("true", "false"):
                    assert sum(f"k_ppc_partial<{dt}, {P}, {lab}>" in r["name"] for r in mine) == 1, (alt, dt, P, lab)
        assert sum("k_ppc_fold" in r["name"] for r in mine) == 1 and sum("k_ppc_moments" in r["name"] for r in mine) == 1
        assert len(mine) == 28
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert all(r["lds"] <= 64 * 1024 for r in mine)
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)


# ---- the Python face ---------------------------------------------------------------------------------------------------------------------------
def test_no_gpu_means_loud_failure_not_fallback():
    import logreg_amd as la
    if la.device_count() > 0:  # with a device the same call gets as far as its argument checks
        with pytest.raises(TypeError):
            la.PredictiveCheck(None)
        return
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        la.PredictiveCheck(None)


def test_check_is_keyword_only_between_rank_and_loo():
    import logreg_amd as la
    params = inspect.signature(la.mcmc).parameters
    assert params["check"].kind is inspect.Parameter.KEYWORD_ONLY and params["check"].default is None
    names = list(params)
    assert names[names.index("rank") + 1] == "check" and names[names.index("check") + 1] == "loo" and names[-3:] == ["covariance", "marginals", "predictive"]
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, check=object())
    assert "PredictiveCheck" in la.__all__ and "ppc_from_table" in la.__all__


def _decided_equal(got_bits, ref):
    ok = ~ref["undecided"]
    return np.array_equal(got_bits[ok], ref["rep"][ok])


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_cpu_double_equals_the_reference_on_decided_pairs(dtype, pscale):
    """tests/host/lr_cpu_twin_ppc.c through the Python face: the replicate of every decided pair, the counts as the popcount of its own
    bits per group, the deviances within the reference's bounds."""
    import logreg_amd as la
    import twin_ppc
    r, p, S = 257, 8, 65
    ref = pc.reference(r, p, S, dtype)
    L = twin_ppc.install()
    try:
        model = la.LogReg(ref["X"], ref["y"], np.ones(p), dtype=dtype)
        groups = pc.groups_for(r, 7)
        acc = la.PredictiveCheck(model, groups=groups, seed=pc.SEED, n_groups=7)
        counts, dev, bits = acc.terms(ref["B"], first_index=pc.FIRST)
        rep = ppr.unpack(bits, r)
        assert _decided_equal(rep, ref) and np.array_equal(counts, ppr.counts_of(rep, groups, 7))
        for k, lab in ((0, ref["y"] > 0.5), (1, rep)):
            D, bound = ppr.deviance(ref["pv"], lab)
            assert np.all(np.abs(dev[:, k] - D) <= bound), (k, np.max(np.abs(dev[:, k] - D) / bound))
        acc.close()
        model.close()
    finally:
        twin_ppc.uninstall()


def test_python_face_on_the_cpu_double(pima, pscale):
    """tests/twin_ppc.py: every refusal; update in any cuts gives the tables of a host recount of terms; reset; a non-finite draw is
    counted and consumes its index; mcmc(..., check=acc) equals feeding the kept draws by hand."""
    import logreg_amd as la
    from logreg_amd import _lib
    import twin
    import twin_ppc
    X, y = pima
    n = X.shape[0]
    L0 = twin.install()  # a library without the entry points
    try:
        model = la.LogReg(X, y, pscale, dtype="float64")
        assert not hasattr(L0, "lr_ppc_create")
        with pytest.raises(la.LogregHipError, match="no predictive-check entry points"):
            la.PredictiveCheck(model)
        model.close()
    finally:
        twin.uninstall()
    L = twin_ppc.install()
    try:
        assert _lib.load() is L and _lib.load_ppc() is L
        model = la.LogReg(X, y, pscale, dtype="float64")
        with pytest.raises(TypeError, match="LogReg"):
            la.PredictiveCheck("model")
        for bad in (1.5, True, "7"):
            with pytest.raises(TypeError, match="seed"):
                la.PredictiveCheck(model, seed=bad)
        for bad in (-1, 2 ** 64):
            with pytest.raises(ValueError, match="seed"):
                la.PredictiveCheck(model, seed=bad)
        with pytest.raises(ValueError, match="y_new without X_new"):
            la.PredictiveCheck(model, y_new=y)
        with pytest.raises(ValueError, match=r"\[r, p\]"):
            la.PredictiveCheck(model, X[:, :7])
        with pytest.raises(ValueError, match="no rows"):
            la.PredictiveCheck(model, X[:0])
        Xb = X.copy()
        Xb[3, 2] = np.inf
        with pytest.raises(ValueError, match="finite"):
            la.PredictiveCheck(model, Xb)
        with pytest.raises(ValueError, match=r"y_new must be \[r\]"):
            la.PredictiveCheck(model, X, y[:-1])
        with pytest.raises(ValueError, match="0 / 1"):
            la.PredictiveCheck(model, X, np.where(np.arange(n) == 4, 2.0, y))
        with pytest.raises(ValueError, match=r"groups must be \[r\]"):
            la.PredictiveCheck(model, groups=np.zeros(n - 1, dtype=int))
        with pytest.raises(ValueError, match="integer labels"):
            la.PredictiveCheck(model, groups=np.full(n, 0.5))
        for bad in (-1, 32):
            with pytest.raises(ValueError, match="0 .. 31"):
                la.PredictiveCheck(model, groups=np.where(np.arange(n) == 0, bad, 0))
        for bad in (0, 33, 2.0, True):
            with pytest.raises(ValueError, match="n_groups"):
                la.PredictiveCheck(model, groups=np.zeros(n, dtype=int), n_groups=bad)
        with pytest.raises(ValueError, match="n_groups"):
            la.PredictiveCheck(model, groups=np.arange(n) % 3, n_groups=2)
        with pytest.raises(ValueError, match="n_groups without groups"):
            la.PredictiveCheck(model, n_groups=2)
        # the library's own refusals, past the face (include/logreg_hip_ppc.h)
        h = ctypes.c_void_p()
        g = np.zeros(n, dtype=np.int32)
        for args, word in (((model.handle, None, None, n - 1, None, 1, 0), "own"), ((model.handle, None, None, 0, None, 1, 0), "positive"),
                           ((model.handle, None, None, n, g.ctypes.data, 0, 0), "G must be"), ((model.handle, None, None, n, g.ctypes.data, 33, 0), "G must be"),
                           ((model.handle, None, None, n, None, 2, 0), "one group"), ((None, None, None, n, None, 1, 0), "NULL")):
            assert L.lr_ppc_create(*args, ctypes.byref(h)) != 0 and word in L.lr_last_error().decode()
        g[5] = 3
        assert L.lr_ppc_create(model.handle, None, None, n, g.ctypes.data, 3, 0, ctypes.byref(h)) != 0 and "groups[5]=3" in L.lr_last_error().decode()

        rng = np.random.default_rng(0)
        import bridge_reference as br
        b, Cv = br.newton_mode(X, y, pscale)
        draws = b + rng.standard_normal((203, 8)) @ np.linalg.cholesky(Cv).T
        groups = (X[:, 1] > np.median(X[:, 1])).astype(int) + 2 * (np.arange(n) % 2)
        acc = la.PredictiveCheck(model, groups=groups, seed=9)
        assert acc.G == 4 and acc.r == n and "n_draws=0" in repr(acc)
        r0 = acc.result()
        assert r0["n_draws"] == 0 and np.all(np.isnan(r0["p_two"])) and r0["n_g"].tolist() == np.bincount(groups).tolist()
        assert r0["t_obs"].tolist() == [int(y[groups == g].sum()) for g in range(4)]
        counts, dev, bits = acc.terms(draws)
        rep = ppr.unpack(bits, n)
        want = ppr.accumulate(counts, dev, rep, r0["n_g"])
        acc.update(draws[:1]).update(draws[1:6]).update(draws[6:39]).update(draws[39:].reshape(4, 41, 8))
        t = acc.tables()
        for k in ("hist", "row_ones", "counts"):
            assert t[k].tobytes() == want[k].tobytes(), k
        assert t["n_draws"] == 203 and np.max(np.abs(t["moments"] - want["moments"]) / ppr.moment_bounds(dev)) <= 1.0
        res = acc.result()
        assert np.all(np.abs(res["mean"] - counts.mean(axis=0)) < 1e-12) and np.all(res["p_ge"] + res["p_le"] >= 1.0) and res["dev_p"] == np.mean(dev[:, 1] >= dev[:, 0])
        assert np.array_equal(acc.terms(draws[7:20], first_index=7)[0], counts[7:20]) and acc.terms(draws[:3], bits=False)[2] is None
        for bad in (np.zeros((4, 7)), np.zeros((0, 8)), np.zeros((2, 3, 4, 8))):
            with pytest.raises(ValueError):
                acc.update(bad)
            with pytest.raises(ValueError):
                acc.terms(bad)
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError, match="first_index"):
                acc.terms(draws[:2], first_index=bad)
        acc.reset()
        assert acc.n_draws == 0 and acc.result()["n_draws"] == 0 and int(acc.tables()["hist"].sum()) == 0
        bad = draws[:9].copy()
        bad[4, 2] = np.nan
        rb = acc.update(bad).result()
        assert rb["n_draws"] == 9 and rb["n_nonfinite"] == 1 and rb["n"] == 8 and np.isfinite(rb["dev_rep_mean"])
        c2 = acc.terms(bad)[0]
        assert np.array_equal(np.delete(c2, 4, axis=0), np.delete(counts[:9], 4, axis=0)) and not c2[4].any()  # the draws after it are where they were
        acc.reset()
        unl = la.PredictiveCheck(model, X[:50], seed=9)
        ru = unl.update(draws[:20]).result()
        assert ru["t_obs"].tolist() == [-1] and np.isnan(ru["p_two"][0]) and np.isnan(ru["dev_p"]) and np.isnan(ru["dev_obs_mean"]) and np.isfinite(ru["dev_rep_mean"])
        unl.close()

        # mcmc(..., check=acc) equals feeding the kept draws by hand
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.tile(b, (6, 1))
        for wrong in ("yes", la.Autocorr(6, 8, "float64")):
            with pytest.raises(ValueError, match="must be a PredictiveCheck"):
                la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, check=wrong)
        other = la.LogReg(X, y, pscale, dtype="float32")
        foreign = la.PredictiveCheck(other)
        with pytest.raises(ValueError, match="own model"):
            la.mcmc(init, kern, thin=1, iters=2, verb=False, seed=1, check=foreign)
        out, info = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, return_info=True, check=acc, chunk=7)
        assert acc.n_draws == 120 and info["check"]["n_draws"] == 120
        by_hand = la.PredictiveCheck(model, groups=groups, seed=9).update(out)
        for k in ("hist", "row_ones", "counts"):
            assert by_hand.tables()[k].tobytes() == info["check"]["tables"][k].tobytes(), k
        acc.reset()
        summ = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, summary_only=True, check=acc)
        assert summ["check"]["tables"]["hist"].tobytes() == info["check"]["tables"]["hist"].tobytes()  # the same draws without a sample matrix
        plain = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4)
        assert plain.tobytes() == out.tobytes()  # the chains are those of the same call without it
        for a in (acc, by_hand, foreign):
            a.close()
        with pytest.raises(la.LogregHipError, match="closed"):
            acc.update(draws[:2])
        other.close()
        model.close()
    finally:
        twin_ppc.uninstall()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------
def test_host_harness_under_the_sanitizers():
    """tests/host/ppc_harness.cpp on the stub runtime, built under AddressSanitizer + UBSan by tests/host_build.py, a program of its
    own: refusals ahead of any device access, a failing allocation at every allocation of create, accumulate and terms, the sub-batch
    rule."""
    import host_build
    r = host_build.run(host_build.harness("ppc_harness.cpp", "asan"))
    line = host_build.last_line(r)
    print("[ppc]", line)
    assert line.startswith("ppc harness:") and line.endswith(" 0 failures")
