"""The NUTS warm-up on the stepwise engine (include/logreg_hip_adapt_tall.h; kernels: csrc/lr_tall_nuts.h TUNED, csrc/lr_adapt.h) on the MI355X.

1. Replay: every warm-up iteration again through the plain lr_run_nuts(mode = stepwise, iters = 1) with the trace's (eps_t, dmm_t) -- state,
   depth and accept_stat_sum to the same bytes, at every padded width.
2. Teacher-forced adaptation against tests/adapt_reference.py, within its input-derived bounds; the step sizes within
   adapt_tall_cases.EPS_RTOL.
3. Bytes: cut into calls, host against device pointers, a rerun, the second build, an asked slice count.
4. Edges: a NaN start, one chain, adapt_metric = False, W < 20, chain shards, C = 257 at p = 128.
5. End to end on the 5001 x 8 model of tests/golden/nuts_tall_posterior.json, and the Python face's refusals.

Largest step-size deviation measured on the MI355X over adapt_tall_cases.TEACHER x both dtypes: see adapt_tall_cases.EPS_RTOL_MEASURED and
profiles/r26_adapt_tall.txt."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import adapt_reference as ar
import adapt_tall_cases as cases
import nuts_reference as nr
import nuts_tall_cases as ntc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    if logreg_amd.device_count() <= 0:
        pytest.skip("no GPU")
    return logreg_amd


_MODELS = {}


def model_of(la, p, dtype):
    if (p, dtype) not in _MODELS:
        _MODELS[(p, dtype)] = la.LogReg(*cases.data(p, dtype), dtype=dtype)
    return _MODELS[(p, dtype)]


def start_of(Cn, p, dtype):
    return cases.start(Cn, p, cases.rows(p, dtype))


def dmm_at(res, W, dmm0, adapt_metric=True):
    """[W, p]: the metric iteration t ran with, from the metric rows of the trace"""
    init, ends = ar.schedule(W) if adapt_metric else (W, [])
    out = np.tile(np.asarray(dmm0, dtype=np.float64), (W, 1))
    for k, e in enumerate(ends):
        out[e:] = res["metric"][k, 1]
    return out


def plain_iteration(model, state, eps, dmm, t, seed, chain_offset=0, group=0, max_depth=cases.MAX_DEPTH):
    """one lr_run_nuts iteration on the stepwise engine at the warm-up's Philox index -> (state, depth [C], counters [C])"""
    from logreg_amd import _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_nuts(model._L)
    st = np.array(state, dtype=model.np_dtype, order="C")
    Cn = st.shape[0]
    depth = np.zeros((1, Cn), dtype=np.int8)
    cnt = np.zeros(Cn, dtype=NUTS_COUNTERS)
    d = np.ascontiguousarray(dmm, dtype=np.float64)
    opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, iter_offset=_lib.ADAPT_ITER_BASE + t, seed=seed, group=group, mode=_lib.MODE_STEPWISE,
                        on_device=0)
    _lib.check(L.lr_run_nuts(model.handle, st.ctypes.data, float(eps), max_depth, d.ctypes.data, C.byref(opts), None, cnt.ctypes.data, depth.ctypes.data))
    return st, depth[0], cnt


def replay(model, q0, res, W, seed, chain_offset=0, dmm0=None, adapt_metric=True, chains=slice(None), patch=None, group=0):
    """every iteration of the warm-up `res` again through the plain path; -> the number of iterations with a positive acceptance statistic"""
    p = q0.shape[1]
    dm = dmm_at(res, W, np.ones(p) if dmm0 is None else dmm0, adapt_metric)
    moved = 0
    for t in range(W):
        prev = np.array(q0 if t == 0 else res["out"][t - 1], dtype=model.np_dtype)
        if patch is not None:
            prev = patch(prev)
        st, depth, cnt = plain_iteration(model, prev, res["trace"][t, 0], dm[t], t, seed, chain_offset, group)
        assert st[chains].tobytes() == res["out"][t][chains].tobytes(), t
        assert np.array_equal(depth[chains], res["depth"][t][chains]), t
        assert cnt["accept_stat_sum"][chains].tobytes() == res["astat"][t][chains].tobytes(), t
        moved += bool(np.any(res["astat"][t] > 0))
    return moved


@pytest.mark.parametrize("case", cases.REPLAY, ids=cases.case_id)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_every_iteration_is_the_plain_stepwise_iteration(la, dtype, case):
    p, Cn, W = case
    model = model_of(la, p, dtype)
    q0 = start_of(Cn, p, dtype)
    res = cases.warm(model, q0, W, seed=5)
    init, ends = ar.schedule(W)
    assert res["info"]["windows"] == len(ends) == res["info"]["n_windows"] and res["info"]["iterations"] == W
    if ends:
        assert not np.array_equal(res["dmm"], np.ones(p))  # the metric changed under way
    assert res["state"].tobytes() == res["out"][-1].tobytes()
    moved = replay(model, q0, res, W, seed=5)
    print("REPLAY %s %s moving %d of %d" % (dtype, cases.case_id(case), moved, W))
    assert moved > W // 2
    cnt = res["counters"]
    assert np.allclose(cnt["accept_stat_sum"], res["astat"].sum(axis=0), rtol=1e-13) and np.array_equal(cnt["depth_sum"], np.abs(res["depth"].astype(np.int64)).sum(axis=0))


@pytest.mark.parametrize("case", cases.TEACHER, ids=cases.case_id)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_teacher_forced_adaptation(la, dtype, case):
    p, Cn, W = case
    model = model_of(la, p, dtype)
    res = cases.warm(model, start_of(Cn, p, dtype), W, seed=17)
    tf = ar.teacher_forced(res["astat"], res["out"], W, np.ones(p))
    tr = res["trace"]
    err = np.abs(tr[:, 1] - tf["abar"])
    assert np.all(err <= tf["tol_abar"]), (np.max(err), np.max(tf["tol_abar"]))
    assert np.array_equal(tr[:, 3], tf["window"]) and np.array_equal(tr[:, 4], tf["n"])
    assert res["info"] == {"iterations": W, "metric_skipped": tf["skipped"], "windows": len(tf["metric"]), "n_windows": len(tf["metric"])}
    for k, mt in enumerate(tf["metric"]):
        var, dmm = res["metric"][k]
        assert np.array_equal(np.isfinite(var) & (var > 0), ~mt["skipped"])
        ok = ~mt["skipped"]
        assert np.all(np.abs(var - mt["var"])[ok] <= mt["tol_var"][ok]), (k, np.max((np.abs(var - mt["var"]) / mt["tol_var"])[ok]))
        assert np.all(np.abs(dmm - mt["dmm"]) <= mt["tol_dmm"]), (k, dmm, mt["dmm"])
    assert np.all(np.abs(res["dmm"] - tf["dmm"]) <= (tf["metric"][-1]["tol_dmm"] if tf["metric"] else 0.0))
    dev = cases.step_size_deviation(res, tf)
    print("DEV %s %s step-size deviation %.3e abar %.3e of tol %.3e moving %d of %d" % (dtype, cases.case_id(case), dev, np.max(err), np.max(tf["tol_abar"]),
                                                                                      int(np.sum(tr[:, 1] > 0)), W))
    assert dev <= cases.EPS_RTOL, dev
    assert tr[0, 0] == 1.0 and np.sum(tr[:, 1] > 0) > W // 2  # from eps0 = 1; most iterations move


@pytest.mark.parametrize("dtype,p", [("float32", 8), ("float64", 65)])
def test_cut_invariance_and_determinism(la, dtype, p):
    import altlib
    Cn, W = 65, 40
    model = model_of(la, p, dtype)
    q0 = start_of(Cn, p, dtype)
    one = cases.warm(model, q0, W, seed=23)
    assert one["info"]["windows"] == 1
    for name, kw in (("1 + 7 + 32", dict(cuts=[1, 7, 32])), ("device pointers", dict(on_device=True)), ("device pointers in pieces", dict(on_device=True, cuts=[1, 7, 32])),
                     ("twice over", dict())):
        assert cases.same_bytes(one, cases.warm(model, q0, W, seed=23, **kw)) is None, name
    assert cases.same_bytes(one, cases.warm(model, q0, W, seed=24)) is not None
    altlib.install()  # the second build of the same sources
    try:
        m_alt = la.LogReg(*cases.data(p, dtype), dtype=dtype)
        alt = cases.warm(m_alt, q0, W, seed=23)
        m_alt.close()
    finally:
        altlib.uninstall()
    assert cases.same_bytes(one, alt) is None


@pytest.mark.parametrize("dtype,p,group", [("float64", 17, 4), ("float32", 33, 3)])
def test_an_asked_slice_count_replays_at_the_same_count(la, dtype, p, group):
    """601 rows in 4 asked slices, 100 rows in 3: the last slice is the shorter one"""
    Cn, W = 3, 40
    model = model_of(la, p, dtype)
    q0 = start_of(Cn, p, dtype)
    res = cases.warm(model, q0, W, seed=27, group=group)
    assert replay(model, q0, res, W, seed=27, group=group) > W // 2
    assert cases.same_bytes(res, cases.warm(model, q0, W, seed=27)) is not None  # (another slicing is another summation order)


@pytest.mark.parametrize("dtype,p", [("float64", 8), ("float32", 128)])
def test_a_nan_start_touches_its_own_chain_and_coordinate_only(la, dtype, p):
    Cn, W, bad, j = 65, 40, 5, 1
    model = model_of(la, p, dtype)
    q0 = start_of(Cn, p, dtype)
    q0[bad, j] = np.nan
    res = cases.warm(model, q0, W, seed=29)  # (the call returns: an iteration is bounded whatever the tally says)
    assert np.all(res["astat"][:, bad] == 0.0) and np.all(np.isnan(res["out"][:, bad, j]))
    others = np.delete(np.arange(Cn), bad)
    abar, tol = ar.abar_of(res["astat"])
    assert np.all(np.abs(res["trace"][:, 1] - abar) <= tol) and np.all(np.abs(res["trace"][:, 1] - res["astat"][:, others].sum(axis=1) / Cn) <= tol)
    var, dmm = res["metric"][0]
    assert not np.isfinite(var[j]) and dmm[j] == 1.0 and res["dmm"][j] == 1.0  # the coordinate's variance is non-finite, its dmm kept
    assert np.all(np.isfinite(np.delete(var, j))) and np.all(np.delete(res["dmm"], j) != 1.0)
    assert res["info"]["metric_skipped"] == 1 and res["info"]["windows"] == 1
    # The other chains are what they are beside a finite neighbour: every iteration replayed through the plain path with this run's
    # (eps_t, dmm_t) from this run's previous states, the NaN replaced by a finite number -- a run of its own from a finite start would
    # have another eps sequence (tests/test_gpu_adapt.py).

    def finite(prev):
        prev = prev.copy()
        prev[bad, j] = 0.01
        return prev
    assert replay(model, q0, res, W, seed=29, chains=others, patch=finite) > W // 2


def test_one_chain_no_metric_short_warmups_and_chain_shards(la):
    p, W = 8, 150
    model = model_of(la, p, "float64")
    # C = 1: the window's n is its length, n - 1 = 24
    q1 = start_of(1, p, "float64")
    one = cases.warm(model, q1, W, seed=31)
    assert one["trace"][99, 4] == 25 and one["trace"][99, 3] == 0 and one["trace"][100, 3] == -1
    mt = ar.metric_of(one["out"][75:100], np.ones(p))
    assert np.all(np.abs(one["metric"][0, 0] - mt["var"]) <= mt["tol_var"])
    # adapt_metric = False leaves dmm0
    d0 = np.linspace(2000.0, 9000.0, p)
    q0 = start_of(9, p, "float64")
    fixed = cases.warm(model, q0, 40, seed=31, dmm0=d0, adapt_metric=False)
    assert fixed["dmm"].tobytes() == d0.tobytes() and fixed["info"]["n_windows"] == 0 == fixed["info"]["windows"] and np.all(fixed["trace"][:, 3] == -1)
    assert replay(model, q0, fixed, 40, seed=31, dmm0=d0, adapt_metric=False) > 20
    tf = ar.teacher_forced(fixed["astat"], fixed["out"], 40, d0, adapt_metric=False)
    assert cases.step_size_deviation(fixed, tf) <= cases.EPS_RTOL
    # W < 20: the step size alone
    short = cases.warm(model, q0, 19, seed=33)
    assert short["info"]["n_windows"] == 0 and np.all(short["trace"][:, 3] == -1) and short["dmm"].tobytes() == np.ones(p).tobytes()
    assert cases.step_size_deviation(short, ar.teacher_forced(short["astat"], short["out"], 19, np.ones(p))) <= cases.EPS_RTOL
    # shards at chain_offset 1, 2, 3 draw the streams of the global chain ids: iteration 0 (eps0 and dmm0: nothing pooled yet) is the whole
    # run's, and every later iteration is the plain path's at that offset with the shard's own (eps_t, dmm_t)
    whole = cases.warm(model, q0, 30, seed=37)
    for off in (1, 2, 3):
        sh = cases.warm(model, q0[off:off + 5], 30, seed=37, chain_offset=off)
        assert sh["out"][0].tobytes() == whole["out"][0][off:off + 5].tobytes() and sh["astat"][0].tobytes() == whole["astat"][0][off:off + 5].tobytes()
        assert sh["out"][1:].tobytes() != whole["out"][1:, off:off + 5].tobytes()  # a shard adapts by itself
        assert replay(model, q0[off:off + 5], sh, 30, seed=37, chain_offset=off) > 15


def test_it_works_on_the_tall_model_from_eps_1_and_the_unit_metric(la):
    """64 chains, W = 150, max_depth 6, then 200 sampling iterations through mcmc(res.state, res.kernel, mode="stepwise").  The bands come from
    the CPU (tools/adapt_tall_cpu_bands.py: adapt_reference.py driving the NumPy NUTS on the same model, 5 seeds; figures in
    profiles/r26_adapt_tall.txt): 2 x the reference's own spread around 1 for pre_j / var_golden_j, and around delta for the sampling run's
    mean acceptance statistic.  The means: the bound of tests/test_gpu_nuts_tall.py's posterior test."""
    g = load_golden("nuts_tall_posterior.json")
    bands = load_golden("adapt_tall_bands.json")
    ref = g["pooled"]
    X, y, ps = ntc.POSTERIOR_MODEL()
    model = la.LogReg(X, y, ps, dtype="float32")
    q0 = np.array(g["map"]) + np.array(g["laplace_sd"]) * np.random.default_rng(41).standard_normal((64, 8))
    res = la.nuts_warmup_stepwise(model.lpost, model.glp, q0, 150, max_depth=6, seed=43)
    assert res.trace[0, 0] == 1.0 and res.info["windows"] == 1 and res.info["metric_skipped"] == 0 and res.kernel.params["eps"] == res.eps
    out, info = la.mcmc(res.state, res.kernel, thin=1, iters=200, verb=False, seed=47, return_info=True, mode="stepwise")
    summ = la.summarise(out)
    z = (summ["mean"] - np.array(ref["mean"])) / np.hypot(summ["mcse"], ref["mcse"])
    ratio = res.pre / np.array(ref["sd"]) ** 2
    acc = float(np.mean(info["mean_accept_stat"]))
    print("TALL eps %.4g ratio %s accept %.4f depth %.3f z %s divergent %d" % (res.eps, np.round(ratio, 3), acc, float(np.mean(info["mean_depth"])), np.round(z, 2),
                                                                              int(info["divergent"].sum())))
    assert info["divergent"].sum() == 0
    assert np.max(np.abs(z)) < 4.2
    assert np.all(np.abs(ratio - 1.0) <= 2.0 * bands["ratio_spread"]), (ratio, bands["ratio_spread"])
    assert abs(acc - 0.8) <= 2.0 * bands["accept_spread"], (acc, bands["accept_spread"])
    model.close()


def test_the_python_face_sends_each_shape_to_its_path(la, pima, pscale):
    X, y = pima
    fused = la.LogReg(X, y, pscale, dtype="float32")
    with pytest.raises(la.LogregHipError, match="lr_adapt_create"):  # the hint: the fused path takes this shape
        la.nuts_warmup_stepwise(fused.lpost, fused.glp, np.zeros((4, 8)), 20)
    fused.close()
    wide = la.LogReg(*nr.synthetic_model(40, 100, 140), dtype="float32")
    with pytest.raises(la.LogregHipError, match="p = 40 > 32"):  # as before
        la.nuts_warmup(wide.lpost, wide.glp, np.zeros((4, 40)), 20)
    res = la.nuts_warmup_stepwise(wide.lpost, wide.glp, 0.01 * np.ones((4, 40)), 20, max_depth=4, seed=3, keep=True)
    assert res.draws.shape == (20, 4, 40) and res.dmm.shape == (40,) and res.info["iterations"] == 20 and res.state.tobytes() == res.draws[-1].astype(np.float64).tobytes()
    wide.close()
