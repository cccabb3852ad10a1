"""Rank-normalised split-R-hat, bulk and tail ESS (include/logreg_hip_rank.h, logreg_amd/rankdiag.py) -- everything that can be checked
without a GPU: the reference (tests/rank_reference.py) on hand-computed ranks, against scipy and against the theory of AR(1) chains, the
two cases the classical R-hat is blind to, the ABI tables and the build gates with the new kernels in both libraries, the Python face on
the CPU double (tests/twin_rank.py), and the host harness under the sanitizers."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

from conftest import REPO
import rank_cases as cases
import rank_reference as rr

WANT = ["lr_rank_accumulate", "lr_rank_create", "lr_rank_destroy", "lr_rank_ranks", "lr_rank_reset", "lr_rank_result"]
# ess_bulk / (S (1 - phi) / (1 + phi)) of 8 AR(1) chains of 1000 steps: (smallest, largest) of the reference over seeds 0 .. 49, rounded
# outwards (profiles/r28_rank.txt section 2)
AR_BAND = {0.0: (0.91, 1.04), 0.5: (0.85, 1.10), 0.9: (0.70, 1.24)}


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def test_reference_ranks_on_twelve_hand_computed_values_with_ties_and_signed_zeros():
    #            sorted: -2 | -0 0 0 | 0.5 0.5 | 1 | 3 3 3 3 | 7        positions 1 | 2-4 | 5-6 | 7 | 8-11 | 12
    x = np.array([3.0, -0.0, 0.5, 7.0, 3.0, 0.0, -2.0, 3.0, 0.5, 1.0, 0.0, 3.0])
    r = np.array([9.5, 3.0, 5.5, 12.0, 9.5, 3.0, 1.0, 9.5, 5.5, 7.0, 3.0, 9.5])
    assert np.array_equal(rr.twice_ranks(x), (2 * r).astype(np.int64))
    assert np.array_equal(rr.twice_ranks(x.reshape(6, 2)), (2 * r).astype(np.int64).reshape(6, 2))
    med, q05, q95 = rr.order_stats(x.reshape(6, 2))
    assert med == 0.75 and q05 == -2.0 and q95 == 3.0  # (x_(6) + x_(7)) / 2; indices 11 // 20 = 0 and 19 * 11 // 20 = 10
    f = np.abs(x - med)  # 2.25 .75 .25 6.25 2.25 .75 2.75 2.25 .25 .25 .75 2.25
    rf = np.array([8.5, 5.0, 2.0, 12.0, 8.5, 5.0, 11.0, 8.5, 2.0, 2.0, 5.0, 8.5])
    assert np.array_equal(rr.twice_ranks(f), (2 * rf).astype(np.int64))
    z = rr.z_of(rr.twice_ranks(x), 12)
    import statistics
    assert abs(z[6] - statistics.NormalDist().inv_cdf(0.625 / 12.25)) < 1e-14 and abs(z[3] + z[6]) < 1e-14  # r = 1 and r = 12 of 12


def test_reference_ranks_and_z_against_scipy():
    import scipy.special
    import scipy.stats
    for shape in cases.SHAPES[:3]:
        for kind in cases.RANK_KINDS:
            for dtype in cases.DTYPES:
                x = cases.draws(shape, kind, dtype)[:shape[0] // 2 * 2, :, 0]
                r2 = rr.twice_ranks(x)
                assert np.array_equal(r2, np.rint(2 * scipy.stats.rankdata(x.ravel() + 0.0, method="average")).astype(np.int64).reshape(x.shape)), (shape, kind, dtype)
                u = (r2 * 0.5 - 0.375) / (x.size + 0.25)
                assert np.max(np.abs(rr.z_of(r2, x.size) - scipy.special.ndtri(u))) < 4e-15
    p = np.concatenate([np.linspace(1e-9, 1 - 1e-9, 100001), 10.0 ** -np.arange(3.0, 300.0, 7.0), [0.075, 0.925, 0.0750001, 0.07499]])
    want = scipy.special.ndtri(p)
    assert np.max(np.abs(rr.ndtri(p) - want) / np.maximum(1.0, np.abs(want))) < 4e-15


@pytest.mark.parametrize("phi", sorted(AR_BAND))
def test_reference_ess_of_ar1_chains_is_the_theorys_within_the_measured_band(phi):
    lo, hi = AR_BAND[phi]
    for seed in range(6):
        x = rr.ar1(np.random.default_rng([seed, int(phi * 10)]), 1000, 8, phi)
        c = rr.column(x, 255)
        ratio = c["ess_bulk"] / (8000 * (1 - phi) / (1 + phi))
        print(f"[rank] AR(1) phi {phi} seed {seed}: ess_bulk / theory {ratio:.4f}, ess_tail {c['ess_tail']:.0f}, rhat {c['rhat']:.4f}")
        assert lo <= ratio <= hi and c["ess_tail"] > 0


def blind_cases():
    rng = np.random.default_rng(0)
    wide = rng.standard_normal((400, 8))
    wide[:, 0] *= 3
    cauchy = rng.standard_cauchy((400, 8))
    cauchy[:, 0] += 3
    return wide, cauchy


def test_reference_sees_what_the_classical_split_rhat_is_blind_to():
    import logreg_amd as la
    wide, cauchy = blind_cases()
    for x, row in ((wide, "rhat_tail"), (cauchy, "rhat_bulk")):
        classical = rr.classical_split_rhat(x)
        c = rr.column(x, 63)
        print(f"[rank] classical split-R-hat {classical:.4f}, rank-normalised: bulk {c['rhat_bulk']:.4f}, folded {c['rhat_tail']:.4f}")
        assert classical < 1.01 and c[row] > 1.05 and c["rhat"] >= c[row]
        assert abs(la.split_rhat(x[:, :, None])[0] - classical) < 1e-12  # the R-hat the package ships is that classical one


def test_reference_edge_cases():
    x = cases.draws((64, 5, 3), "smooth", "float64")
    for n in (0, 1, 2, 3):
        T, _ = rr.table(x[:n], 63)
        assert np.all(np.isnan(T[:11])) and np.all(T[11] == 0)
    y = x.copy()
    y[3, 1, 2] = np.nan
    y[9, 0, 2] = -np.inf
    T, _ = rr.table(y, 63)
    assert np.all(np.isnan(T[:11, 2])) and T[11, 2] == 2 and np.all(np.isfinite(T[:5, :2]))
    assert T[:, :2].tobytes() == rr.table(x, 63)[0][:, :2].tobytes()
    T, _ = rr.table(cases.draws((64, 5, 3), "equal", "float32"), 63)
    assert np.all(np.isnan(T[:8, 0])) and np.all(T[8:11, 0] == 1.5)
    odd = rr.table(np.concatenate([x, 1e9 + x[:1]]), 63)[0]  # an odd last step is ignored
    assert odd.tobytes() == rr.table(x, 63)[0].tobytes()
    # the lag cap: a slowly mixing chain runs out of lags at max_lag = 7 and is flagged; with 255 lags it is not
    slow = rr.ar1(np.random.default_rng(3), 2000, 4, 0.97)
    assert rr.column(slow, 7)["capped_bulk"] == 1.0 and rr.column(slow, 255)["capped_bulk"] == 0.0
    assert rr.column(slow, 7)["pairs_bulk"] == 4.0 and rr.column(slow, 7)["ess_bulk"] > rr.column(slow, 255)["ess_bulk"]


# ---- ABI and build ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_table_matches_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_rank.h") == WANT == sorted(_lib.RANK_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.PG_SYMBOLS,
                  _lib.BRIDGE_SYMBOLS):
        assert not set(WANT) & set(other)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38  # logreg_hip.h's set stays as pinned
    hdr = open(os.path.join(REPO, "include", "logreg_hip_rank.h")).read()
    assert int(re.search(r"#define LR_RANK_ROWS (\d+)", hdr).group(1)) == _lib.RANK_ROWS == len(rr.ROWS) == 15
    assert int(re.search(r"#define LR_RANK_MAX_LAG (\d+)", hdr).group(1)) == _lib.RANK_MAX_LAG == 255
    assert re.search(r"#define LR_RANK_MAX_DRAWS \(1ll << (\d+)\)", hdr).group(1) == "24" and _lib.RANK_MAX_DRAWS == 1 << 24
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_rank_\w+)", exported))) == WANT, path
    assert _lib.load_rank() is _lib.load()  # binds on first use
    src = build._sources()
    assert os.path.join(build.INCLUDE, "logreg_hip_rank.h") in src and os.path.join(build.CSRC, "lr_rank.h") in src and os.path.join(build.CSRC, "lr_rank_math.h") in src


def test_still_13_units_and_the_rank_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        objs = b.unit_objects(alt)
        assert len(objs) == 13
        mine = [r for r in b.kernel_resources(alt=alt) if "k_rank_" in r["name"]]
        assert {r["unit"] for r in mine} == {"lr_api"}
        for k in ("k_rank_gather<float>", "k_rank_gather<double>", "k_rank_lookup<false>", "k_rank_lookup<true>", "k_rank_transform<false>", "k_rank_transform<true>", "k_rank_fold", "k_rank_sort_tile", "k_rank_merge_global",
                  "k_rank_quant", "k_rank_lag", "k_rank_partial", "k_rank_final"):
            assert sum(k in r["name"] for r in mine) == 1, (alt, k)
        assert len(mine) == 13
        assert all(r["scratch"] == 0 for r in mine), [(r["name"], r["scratch"]) for r in mine if r["scratch"]]
        assert all(r["lds"] <= 64 * 1024 for r in mine) and max(r["lds"] for r in mine) == 64 * 1024  # one tile of 8192 keys
        assert isa_gate.scan_paths(objs) == []
        b.exec_prologue_gate(strict=True, verbose=False, alt=alt)
    b.resource_gate(strict=True, verbose=False)  # (the second build may use scratch in older kernels: its gate only reports)


# ---- the Python face ---------------------------------------------------------------------------------------------------------------------------
def test_no_gpu_means_loud_failure_not_fallback():
    import logreg_amd as la
    acc = la.RankDiagnostics(5, 3, 8)
    if la.device_count() > 0:
        return
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        acc.update(np.zeros((2, 5, 3)))
    with pytest.raises(la.LogregHipError, match="no CPU fallback"):
        acc.result()


def test_rank_is_keyword_only_after_autocorr():
    import logreg_amd as la
    params = inspect.signature(la.mcmc).parameters
    assert params["rank"].kind is inspect.Parameter.KEYWORD_ONLY and params["rank"].default is None
    names = list(params)
    assert names[names.index("autocorr") + 1] == "rank" and names[-3:] == ["covariance", "marginals", "predictive"]
    with pytest.raises(ValueError, match="fused kernel"):
        la.mcmc(np.zeros(2), lambda x: x, thin=1, iters=2, verb=False, rank=object())


def test_constructor_checks_and_the_pure_numpy_helper():
    import logreg_amd as la
    for kw, word in ((dict(max_lag=64), "odd"), (dict(max_lag=257), "odd"), (dict(max_lag=-1), "odd"), (dict(dtype="int32"), "dtype")):
        with pytest.raises(ValueError, match=word):
            la.RankDiagnostics(5, 3, 8, **kw)
    for args in ((0, 3, 8), (5, 0, 8), (5, 3, 0)):
        with pytest.raises(ValueError, match="positive"):
            la.RankDiagnostics(*args)
    with pytest.raises(ValueError, match="beyond the cap"):
        la.RankDiagnostics(4097, 3, 4096)
    assert la.RankDiagnostics(4096, 3, 4096).max_lag == 63
    assert "max_steps=8" in repr(la.RankDiagnostics(5, 3, 8, "float64", max_lag=7))
    T = np.arange(45.0).reshape(15, 3)
    r = la.rank_result_from_table(T, 9, 5, 63)
    assert np.array_equal(r["rhat"], T[2]) and np.array_equal(r["ess_tail"], T[4]) and r["n_nonfinite"].dtype == np.int64 and r["n_used"] == 8 and r["n"] == 9
    assert set(rr.ROWS) <= set(r) and np.array_equal(r["pairs_q95"], T[14]) and r["chains"] == 5
    with pytest.raises(ValueError):
        la.rank_result_from_table(np.zeros((14, 3)), 8, 5, 63)


def test_python_face_on_the_cpu_double():
    """tests/twin_rank.py: the double follows the header with the device's own scalar arithmetic (csrc/lr_rank_math.h: keys, AS 241, the
    finish of the tables), so this is also where that code meets the reference without a GPU: ranks as integers, z and the statistics
    to a few ulps, NaN where the reference has it; refusals; every feeding the same bytes; mcmc(..., rank=acc) equals feeding the kept
    draws by hand."""
    import logreg_amd as la
    from logreg_amd import _lib
    import twin
    import twin_rank
    L0 = twin.install()  # a library without the entry points
    try:
        assert not hasattr(L0, "lr_rank_create")
        with pytest.raises(la.LogregHipError, match="no rank-diagnostics entry points"):
            la.RankDiagnostics(5, 3, 8).update(np.zeros((2, 5, 3)))
    finally:
        twin.uninstall()
    L = twin_rank.install()
    try:
        assert _lib.load() is L and _lib.load_rank() is L
        worst = 0.0
        for shape in cases.SHAPES[:3]:
            for kind in cases.RANK_KINDS + ["ar"]:
                for dtype in cases.DTYPES:
                    x = cases.draws(shape, kind, dtype)
                    n, C, p = shape
                    acc = la.RankDiagnostics(C, p, n, dtype)
                    assert np.all(np.isnan(acc.table()[:11])) and acc.n_draws == 0
                    acc.update(x[:n // 3 + 1]).update(x[n // 3 + 1:])
                    T, (R, margin) = acc.table(), rr.table(x, 63)
                    assert np.array_equal(np.isnan(T), np.isnan(R)), (shape, kind, dtype)
                    for r in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14):
                        assert np.array_equal(T[r], R[r], equal_nan=True), (shape, kind, dtype, rr.ROWS[r])
                    ok = ~np.isnan(R[:5])
                    if ok.any():
                        worst = max(worst, float(np.max(np.abs(T[:5][ok] - R[:5][ok]) / np.abs(R[:5][ok]))))
                    for j in range(p):
                        col = rr.column(x[:, :, j], 63)
                        if "twice_r" in col:
                            r2, z = acc.ranks(j, with_z=True)
                            assert np.array_equal(r2, col["twice_r"]) and np.array_equal(acc.ranks(j, folded=True), col["twice_rf"])
                            assert np.max(np.abs(z - col["z"])) < 4e-15
                    res = acc.result()
                    assert res["n"] == n and res["n_used"] == n // 2 * 2 and res["chains"] == C and res["table"].tobytes() == T.tobytes()
                    with pytest.raises(ValueError, match="exceed max_steps"):
                        acc.update(x[:1])
                    acc.reset()
                    assert acc.n_draws == 0 and np.all(np.isnan(acc.table()[:11]))
                    acc.update(x)
                    assert acc.table().tobytes() == T.tobytes()
                    acc.free()
        print(f"[rank] CPU double against the reference: largest relative error of the statistics {worst:.3e}")
        assert worst < 1e-12
        wide, cauchy = blind_cases()
        acc = la.RankDiagnostics(8, 2, 400, "float64").update(np.stack([wide, cauchy], axis=2))
        res = acc.result()
        assert res["rhat_tail"][0] > 1.05 and res["rhat_bulk"][1] > 1.05 and np.all(la.split_rhat(np.stack([wide, cauchy], axis=2)) < 1.01)
        acc.free()

        # mcmc(..., rank=acc) equals feeding the kept draws by hand
        with open(os.path.join(REPO, "tests", "golden", "pima_xy.json")) as f:
            d = json.load(f)
        with open(os.path.join(REPO, "tests", "golden", "map.json")) as f:
            mp = json.load(f)
        model = la.LogReg(np.array(d["X"]), np.array(d["y"]), np.array(mp["pscale"]), dtype="float64")
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=5, dmm=np.ones(8))
        init = np.tile(np.array(mp["map"]), (6, 1))
        for wrong, word in (("yes", "must be a RankDiagnostics"), (la.Autocorr(6, 8, "float64"), "must be a RankDiagnostics"), (la.RankDiagnostics(5, 8, 20, "float64"), "6 chains"),
                            (la.RankDiagnostics(6, 8, 20, "float32"), "float32"), (la.RankDiagnostics(6, 8, 19, "float64"), "max_steps = 19")):
            with pytest.raises(ValueError, match=word):
                la.mcmc(init, kern, thin=1, iters=20, verb=False, seed=1, rank=wrong)
        rk = la.RankDiagnostics(6, 8, 20, "float64")
        out, info = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, return_info=True, rank=rk, chunk=7)
        by_hand = la.RankDiagnostics(6, 8, 20, "float64").update(out)
        assert rk.n_draws == 20 and info["rank"]["table"].tobytes() == by_hand.table().tobytes() and np.array_equal(rk.ranks(3), by_hand.ranks(3))
        rk.reset()
        summ = la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4, summary_only=True, rank=rk)
        assert summ["rank"]["table"].tobytes() == info["rank"]["table"].tobytes()  # the same draws without a sample matrix
        assert la.mcmc(init, kern, thin=2, iters=20, verb=False, seed=4).tobytes() == out.tobytes()  # the chains are those of the same call without it
        for a in (rk, by_hand):
            a.free()
        model.close()
    finally:
        twin_rank.uninstall()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------
def test_host_harness_under_the_sanitizers():
    """tests/host/rank_harness.cpp on the stub runtime, built under AddressSanitizer + UBSan by tests/host_build.py: every allocation
    of create, accumulate, result and ranks fails in turn."""
    import host_build
    r = host_build.run(host_build.harness("rank_harness.cpp", "asan"))
    line = host_build.last_line(r)
    print("[rank]", line)
    assert line.startswith("rank harness:") and line.endswith(" 0 failures")
