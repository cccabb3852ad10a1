"""The posterior-predictive accumulator on the GPU (include/logreg_hip_predict.h, csrc/lr_predict.h) against tests/predict_reference.py.

Every entry of every table of the test set (tests/predict_cases.py: both dtypes, real widths 3 ... 128, r in {1 ... 4097}, S in {1 ...
262144}, one batch and uneven batches, host and device memory, new rows and the model's own design) is compared with the float64
reference on the same dtype-rounded inputs.

The bounds are measured, not chosen (profiles/r9_predict.txt; `python tests/test_gpu_predict.py --measure` prints the figures):
  float64 model   8 x the largest deviation of the kernel's table from the reference over the whole test set
  float32 model   8 x the largest deviation of the REFERENCE's float32 mode from its float64 mode over the whole test set -- what any
                  float32 evaluation of the formulae costs; the kernel's own deviation is reported beside it
in two figures each: rows 0, 2, 3 (means) absolute, rows 1, 4 (sums of squares) divided by S.  8 x is the repository's convention
(profiles/r8_nuts_reference.txt).
"""
import faulthandler
import sys

import numpy as np
import pytest

import predict_cases as pc
import predict_reference as pr

pytestmark = pytest.mark.gpu

# measured figures (profiles/r9_predict.txt) -> bounds = 8 x
MEASURED = {
    "float64": {"mean": 1.776e-15, "var": 7.245e-16},  # the kernel against the float64 reference
    "float32": {"mean": 5.614e-07, "var": 2.190e-07},  # the reference's float32 mode against its float64 mode
}
BOUND = {dt: {k: 8.0 * v for k, v in d.items()} for dt, d in MEASURED.items()}
CASES = None
_REF = {}


def all_cases():
    global CASES
    if CASES is None:
        CASES = pc.cases()
    return CASES


def reference(case, dtype):
    key = (case["name"], dtype)
    if key not in _REF:
        Xn, yn, B = pc.rounded(case, np.dtype(dtype).type)
        _REF[key] = pr.reference_table(Xn, yn, B, return_info=True)
    return _REF[key]


@pytest.fixture(autouse=True)
def step_timeout():
    """Every step under its own time limit: a step that hangs ends the whole run (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def la():
    import logreg_amd as la
    return la


def run_case(la, case, dtype, how):
    model = la.LogReg(case["X"], case["y"], case["pscale"], dtype=dtype)
    pp = la.PosteriorPredictive(model, case["X_new"], case["y_new"])
    B = case["B"].astype(model.np_dtype)
    pc.feed(la, pp, B, how)
    assert pp.n_draws == B.shape[0]
    t = pp.table()
    pp.close()
    model.close()
    return t


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", pc.NAMES)
def test_every_entry_of_the_table_against_the_reference(la, name, dtype):
    case = next(c for c in all_cases() if c["name"] == name)
    ref, info = reference(case, dtype)
    S = case["B"].shape[0]
    labelled = case["X_new"] is None or case["y_new"] is not None
    if labelled:  # row 2 of the reference is free of underflow on this input
        assert info["min_L"] > 1e-30, info
        assert np.all(ref[2] > 1e-30)
    else:
        assert np.all(np.isnan(ref[2:]))
    tabs = []
    for how in case["batchings"]:
        t = run_case(la, case, dtype, how)
        assert t.shape == ref.shape and np.array_equal(np.isnan(t), np.isnan(ref)), (name, how)
        dm, dv = pc.deviations(t, ref, S)
        print(f"[predict] {name} {dtype} {how}: mean rows {dm:.3e}  variance rows {dv:.3e}")
        assert dm <= BOUND[dtype]["mean"], (name, dtype, how, dm, BOUND[dtype]["mean"])
        assert dv <= BOUND[dtype]["var"], (name, dtype, how, dv, BOUND[dtype]["var"])
        tabs.append(t)
    dm, dv = pc.deviations(tabs[0], tabs[1], S)  # two batchings of the same draws
    assert dm <= BOUND[dtype]["mean"] and dv <= BOUND[dtype]["var"], (name, dtype, dm, dv)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_same_calls_same_bytes_and_both_builds_agree(la, dtype):
    """The same call sequence twice gives identical bytes; the production library and the second build (tests/altlib.py: default
    scheduler, SLP on) give identical bytes -- the arithmetic is spelled out (explicit fma), so flags may not change a result."""
    from logreg_amd import _lib
    import altlib
    picks = [c for c in all_cases() if c["name"] in ("pima_own_r200_S4096", "synthetic_p13_r4097_S255", "synthetic_p47_r1000_S255", "synthetic_p128_r200_S4096",
                                                     "synthetic_p20_r63_S4096_nolabels")]
    assert len(picks) == 5
    for case in picks:
        how = case["batchings"][1]
        a = run_case(la, case, dtype, how)
        b = run_case(la, case, dtype, how)
        assert a.tobytes() == b.tobytes(), case["name"]
        L = altlib.install()
        try:
            _lib.bind_predict(L)
            assert _lib.load() is L
            c = run_case(la, case, dtype, how)
        finally:
            altlib.uninstall()
            _lib.bind_predict(_lib.load())
        assert a.tobytes() == c.tobytes(), case["name"]


def mcmc_runs(la, dtype):
    """HMC on Pima, 64 chains x 40 kept draws in chunks of 16: without `predictive`, with it under summary_only=True, with it and kept
    samples, and a third accumulator fed the kept matrix from the host.  -> everything the test compares"""
    d = pc._golden("pima_xy.json")
    X, y = np.array(d["X"]), np.array(d["y"])
    pscale, map_beta = np.array(pc._golden("map.json")["pscale"]), np.array(pc._golden("map.json")["map"])
    model = la.LogReg(X, y, pscale, dtype=dtype)
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
    C, iters = 64, 40
    init = map_beta + 0.01 * np.random.default_rng(5).standard_normal((C, 8))
    kw = dict(thin=2, iters=iters, verb=False, seed=99, chunk=16)
    plain = la.mcmc(init, kern, summary_only=True, **kw)
    pp = la.PosteriorPredictive(model)
    with_pp = la.mcmc(init, kern, summary_only=True, predictive=pp, **kw)
    mat, info = la.mcmc(init, kern, return_info=True, **kw)
    pp2 = la.PosteriorPredictive(model)
    mat2, info2 = la.mcmc(init, kern, return_info=True, predictive=pp2, **kw)
    pp3 = la.PosteriorPredictive(model).update(mat)
    ref = pr.reference_table(X.astype(model.np_dtype).astype(float), y, mat.astype(np.float64))
    return dict(model=model, plain=plain, with_pp=with_pp, pp=pp, pp2=pp2, pp3=pp3, mat=mat, mat2=mat2, info=info, info2=info2, ref=ref, S=C * iters)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype):
    r = mcmc_runs(la, dtype)
    plain, with_pp, pp, pp2, pp3, S = r["plain"], r["with_pp"], r["pp"], r["pp2"], r["pp3"], r["S"]
    assert with_pp["predictive"] is pp and pp.n_draws == pp2.n_draws == pp3.n_draws == S
    assert set(with_pp) == set(plain) | {"predictive"}
    for key in plain:  # state, statistics, accept rate, plan: exactly the run without `predictive`
        a, b = plain[key], with_pp[key]
        assert (np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) if not isinstance(a, dict) else a == b), key
    assert r["mat"].tobytes() == r["mat2"].tobytes()
    assert np.array_equal(r["info"]["accepts"], r["info2"]["accepts"]) and np.array_equal(r["info"]["state"], r["info2"]["state"])
    assert np.array_equal(r["info"]["state"], plain["state"])  # summary_only and kept-samples runs are the same chains
    for t in (pp.table(), pp2.table(), pp3.table()):
        dm, dv = pc.deviations(t, r["ref"], S)
        print(f"[predict] mcmc {dtype}: mean rows {dm:.3e}  variance rows {dv:.3e}")
        assert dm <= BOUND[dtype]["mean"] and dv <= BOUND[dtype]["var"], (dm, dv)
    assert pp.table().tobytes() == pp2.table().tobytes()  # the same blocks in the same order
    w = pp.waic()
    assert np.isfinite(w["elpd_waic"]) and 0 < w["p_waic"] < 20 and w["se"] > 0
    for q in (pp, pp2, pp3):
        q.close()
    r["model"].close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_nan_draw_makes_the_whole_table_nan_and_reset_clears_it(la, dtype):
    case = next(c for c in all_cases() if c["name"] == "pima_own_r200_S4096")
    model = la.LogReg(case["X"], case["y"], case["pscale"], dtype=dtype)
    pp = la.PosteriorPredictive(model)
    B = case["B"].astype(model.np_dtype)
    bad = B.copy()
    bad[1234, 5] = np.nan
    pp.update(bad)
    assert np.all(np.isnan(pp.table())) and pp.n_draws == 4096
    pp.update(B[:100])  # stays NaN until reset
    assert np.all(np.isnan(pp.table()))
    pp.reset()
    assert pp.n_draws == 0 and np.all(np.isnan(pp.table()))  # empty: NaN by definition
    pp.update(B)
    t = pp.table()
    assert np.all(np.isfinite(t))
    clean = run_case(la, case, dtype, "host")
    assert t.tobytes() == clean.tobytes()
    # a NaN in a later batch, in a coordinate whose x entries are all finite
    bad2 = B[:255].copy()
    bad2[254, 0] = np.nan
    pp.update(bad2)
    assert np.all(np.isnan(pp.table()))
    pp.close()
    model.close()


def test_a_closed_model_is_refused_and_the_accumulator_still_closes(la, pima, pscale):
    """The accumulator reads the model's rows: after model.close(), update() and table() raise instead of touching freed memory, and
    close() (which frees the accumulator's own buffers only) still works."""
    X, y = pima
    model = la.LogReg(X, y, pscale, dtype="float32")
    pp = la.PosteriorPredictive(model).update(np.zeros((4, 8)))
    assert pp.table().shape == (5, 200) and pp.n_draws == 4
    model.close()
    with pytest.raises(la.LogregHipError, match="closed"):
        pp.table()
    with pytest.raises(la.LogregHipError, match="closed"):
        pp.update(np.zeros((4, 8)))
    pp.close()


def test_rows_and_labels_are_the_models_own(la, pima, pscale, map_beta):
    """Loose sanity check: on Pima's own rows, at posterior-like draws around the MAP of tests/golden/map.json, the predictive probability
    lies within a few posterior standard deviations of sigma(x . beta_MAP), and L is pi or 1 - pi according to the model's labels."""
    X, y = pima
    model = la.LogReg(X, y, pscale, dtype="float64")
    B = pr.posterior_like_draws(X, y, pscale, 4096, 11, center=map_beta)
    pp = la.PosteriorPredictive(model).update(B)
    mean, sd = pp.proba()
    t = pp.table()
    at_map = 1 / (1 + np.exp(-X @ map_beta))
    assert np.all(np.abs(mean - at_map) < 3 * sd + 1e-3), float(np.max(np.abs(mean - at_map) / sd))
    assert np.allclose(np.where(y == 1, t[0], 1 - t[0]), t[2], rtol=0, atol=1e-12)
    assert np.allclose(pp.lppd(), np.log(t[2]))
    m2, s2 = la.predict_proba(model, B, X)
    assert np.allclose(m2, mean, rtol=0, atol=1e-12) and np.allclose(s2, sd, rtol=0, atol=1e-10)
    w = la.waic(model, B)
    assert abs(w["elpd_waic"] - pp.waic()["elpd_waic"]) < 1e-9
    # shape errors are refused with a reason
    with pytest.raises(ValueError, match="p=8"):
        pp.update(np.zeros((10, 7)))
    with pytest.raises(ValueError, match="S = 0"):
        pp.update(np.zeros((0, 8)))
    with pytest.raises(la.LogregHipError, match="0/1"):
        from logreg_amd import _lib
        import ctypes as C
        h = C.c_void_p()
        yy = np.array([0.0, 2.0])
        _lib.check(_lib.load_predict().lr_predict_create(model.handle, X[:2].ctypes.data, yy.ctypes.data, 2, C.byref(h)))
    pp.close()
    model.close()


def test_host_draws_one_longer_than_a_staging_piece_give_the_bytes_of_two_updates(la):
    """The one path no case above reaches: host draws that do not fit one staging piece, padded to the kernel width on the way.  One
    `update` with a draw more than a piece is the launch sequence of two `update`s cut at the piece boundary, so the bytes are the same."""
    # draws are staged in pieces of max(1024, 256 MB / (P esize)) draws, P the padded width: p = 100 -> P = 128, 256 MB / (128 x 8 bytes) =
    # 262144 draws.  (A change of the 256 MB needs another shape here.)
    p, piece = 100, 262144
    rng = np.random.default_rng(13)
    X = rng.standard_normal((16, p))
    y = (rng.random(16) < 0.5).astype(np.float64)
    B = 0.05 * rng.standard_normal((piece + 1, p))
    model = la.LogReg(X, y, np.full(p, 2.0), dtype="float64")
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        pp = la.PosteriorPredictive(model)
        s0 = 0
        for S in cuts:
            pp.update(B[s0:s0 + S])
            s0 += S
        assert pp.n_draws == piece + 1
        out.append(pp.table())
        pp.close()
    model.close()
    assert np.all(np.isfinite(out[0])) and np.all((out[0][0] > 0) & (out[0][0] < 1))
    assert out[0].tobytes() == out[1].tobytes()


def measure():
    """Print the four figures of profiles/r9_predict.txt: per dtype, the largest deviation over the whole test set of (a) the kernel's
    table from the float64 reference and (b) the reference's float32 mode from its float64 mode (float32 inputs)."""
    import logreg_amd as la
    fig = {("kernel", dt, k): 0.0 for dt in ("float64", "float32") for k in ("mean", "var")}
    fig.update({("ref32", "float32", k): 0.0 for k in ("mean", "var")})
    for case in all_cases():
        S = case["B"].shape[0]
        for dtype in ("float64", "float32"):
            ref, info = reference(case, dtype)
            for how in case["batchings"]:
                dm, dv = pc.deviations(run_case(la, case, dtype, how), ref, S)
                print(f"kernel {dtype} {case['name']} {how}: mean rows {dm:.3e}  variance rows {dv:.3e}  (reference min L {info['min_L']:.3e})", flush=True)
                fig[("kernel", dtype, "mean")] = max(fig[("kernel", dtype, "mean")], dm)
                fig[("kernel", dtype, "var")] = max(fig[("kernel", dtype, "var")], dv)
        Xn, yn, B = pc.rounded(case, np.float32)
        dm, dv = pc.deviations(pr.reference_table(Xn, yn, B, mode="float32"), reference(case, "float32")[0], S)
        print(f"reference float32 mode vs float64 mode {case['name']}: mean rows {dm:.3e}  variance rows {dv:.3e}", flush=True)
        fig[("ref32", "float32", "mean")] = max(fig[("ref32", "float32", "mean")], dm)
        fig[("ref32", "float32", "var")] = max(fig[("ref32", "float32", "var")], dv)
    for dtype in ("float64", "float32"):  # the draws of the mcmc test belong to the test set
        r = mcmc_runs(la, dtype)
        for t in (r["pp"].table(), r["pp2"].table(), r["pp3"].table()):
            dm, dv = pc.deviations(t, r["ref"], r["S"])
            print(f"kernel {dtype} mcmc: mean rows {dm:.3e}  variance rows {dv:.3e}", flush=True)
            fig[("kernel", dtype, "mean")] = max(fig[("kernel", dtype, "mean")], dm)
            fig[("kernel", dtype, "var")] = max(fig[("kernel", dtype, "var")], dv)
        if dtype == "float32":
            X32 = pc.rounded(dict(X=np.array(pc._golden("pima_xy.json")["X"]), y=None, X_new=None, B=r["mat"].reshape(-1, 8)), np.float32)[0]
            dm, dv = pc.deviations(pr.reference_table(X32, np.array(pc._golden("pima_xy.json")["y"]), r["mat"].astype(np.float64), mode="float32"), r["ref"], r["S"])
            print(f"reference float32 mode vs float64 mode mcmc: mean rows {dm:.3e}  variance rows {dv:.3e}", flush=True)
            fig[("ref32", "float32", "mean")] = max(fig[("ref32", "float32", "mean")], dm)
            fig[("ref32", "float32", "var")] = max(fig[("ref32", "float32", "var")], dv)
    for k, v in fig.items():
        print("FIGURE", *k, f"{v:.3e}")


if __name__ == "__main__":
    import os
    if sys.argv[1:] != ["--measure"]:
        sys.exit("usage: python tests/test_gpu_predict.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
