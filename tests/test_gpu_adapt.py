"""The NUTS warm-up (include/logreg_hip_adapt.h; kernels in csrc/lr_nuts.h TUNED and csrc/lr_adapt.h) on the MI355X.

1. The tuned kernel is the plain kernel: every warm-up iteration replayed by a one-iteration lr_run_nuts with the trace's (eps_t, dmm_t).
2. Teacher-forced adaptation: from the device's own acceptance statistics and states the NumPy restatement (tests/adapt_reference.py)
   recomputes abar_t, the step sizes, log_eps_bar, every window's variance and metric, the final step.
3. Cut invariance and determinism: one call, 1 + 7 + 142, 150 single calls, device pointers, twice over, the second build -- bytes.
4. Edge rules: a NaN start, one chain, adapt_metric = False, chain shards.
5. It works, on Pima, from eps = 1 and the unit metric.

The relative tolerance of the step-size comparison (adapt_cases.EPS_RTOL) is 8 x the largest deviation measured on the MI355X over
adapt_cases.CASES x both dtypes: 9.340e-15 measured (float64, C = 1025, p = 8, W = 260), recorded in profiles/r18_adapt.txt."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import adapt_cases as cases
import adapt_reference as ar

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
        X, y, ps = cases.data(p)
        _MODELS[(p, dtype)] = la.LogReg(X, y, ps, dtype=dtype)
    return _MODELS[(p, dtype)]


def dmm_at(res, W, dmm0):
    """[W, p]: the metric iteration t ran with, from the metric rows of the trace"""
    init, ends = ar.schedule(W)
    out = np.tile(np.asarray(dmm0, dtype=np.float64), (W, 1))
    for k, e in enumerate(ends[:len(res["metric"])]):  # (adapt_metric = False: no window, no row)
        out[e:] = res["metric"][k, 1]
    return out


def plain_iteration(la, model, state, eps, dmm, t, seed, chain_offset=0, max_depth=cases.MAX_DEPTH):
    """one lr_run_nuts iteration at the warm-up's Philox index -> (state, depth [C], counters [C])"""
    from logreg_amd import _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_nuts(model._L)
    st = np.array(state, dtype=model.np_dtype, order="C")
    Cn = st.shape[0]
    depth = np.zeros((1, Cn), dtype=np.int8)
    cnt = np.zeros(Cn, dtype=NUTS_COUNTERS)
    d = np.ascontiguousarray(dmm, dtype=np.float64)
    opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, iter_offset=_lib.ADAPT_ITER_BASE + t, seed=seed, group=0, mode=_lib.MODE_AUTO, on_device=0)
    _lib.check(L.lr_run_nuts(model.handle, st.ctypes.data, float(eps), max_depth, d.ctypes.data, C.byref(opts), None, cnt.ctypes.data, depth.ctypes.data))
    return st, depth[0], cnt


def replay(la, model, q0, res, W, seed, chain_offset=0, dmm0=None, chains=slice(None), patch=None):
    """every iteration of the warm-up `res` again through the plain kernel; returns the number of iterations whose acceptance statistic
    was positive (so that the comparison is not one of rejected trees only)"""
    p = q0.shape[1]
    dm = dmm_at(res, W, np.ones(p) if dmm0 is None else dmm0)
    moved = 0
    for t in range(W):
        prev = np.array(q0 if t == 0 else res["out"][t - 1], dtype=model.np_dtype)
        if patch is not None:
            prev = patch(prev)
        st, depth, cnt = plain_iteration(la, model, prev, res["trace"][t, 0], dm[t], t, seed, chain_offset)
        assert st[chains].tobytes() == res["out"][t][chains].tobytes(), t
        assert np.array_equal(depth[chains], res["depth"][t][chains]), t
        assert cnt["accept_stat_sum"][chains].tobytes() == res["astat"][t][chains].tobytes(), t
        moved += bool(np.any(res["astat"][t] > 0))
    return moved


@pytest.mark.parametrize("dtype,Cn,p", [("float32", 1, 8), ("float32", 3, 20), ("float64", 1, 16), ("float64", 3, 3)])
def test_the_tuned_kernel_is_the_plain_kernel(la, dtype, Cn, p):
    W = 150
    model = model_of(la, p, dtype)
    q0 = cases.start(Cn, p)
    res = cases.warm(model, q0, W, seed=5)
    assert res["info"]["windows"] == 1 and not np.array_equal(res["dmm"], np.ones(p))  # the metric changed under way
    assert res["state"].tobytes() == res["out"][-1].tobytes()
    moved = replay(la, model, q0, res, W, seed=5)
    assert moved > W // 2
    cnt = res["counters"]
    assert np.allclose(cnt["accept_stat_sum"], res["astat"].sum(axis=0), rtol=1e-13) and np.array_equal(cnt["depth_sum"], np.abs(res["depth"].astype(np.int64)).sum(axis=0))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_teacher_forced_adaptation(la, dtype, case):
    Cn, p, W = case
    model = model_of(la, p, dtype)
    res = cases.warm(model, cases.start(Cn, p), W, seed=17)
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
    dev = max(np.max(np.abs(tr[:, 0] - tf["eps"]) / tf["eps"]), np.max(np.abs(tr[:, 2] - tf["log_eps_bar"]) / np.maximum(np.abs(tf["log_eps_bar"]), 1.0)),
              abs(res["eps"] - tf["final"]) / tf["final"])
    print("DEV %s %s step-size deviation %.3e abar %.3e of tol %.3e moving %d of %d" % (dtype, cases.case_id(case), dev, np.max(err), np.max(tf["tol_abar"]),
                                                                                      int(np.sum(tr[:, 1] > 0)), W))
    assert dev <= cases.EPS_RTOL, dev
    assert tr[0, 0] == 1.0 and np.sum(tr[:, 1] > 0) > W // 2  # from eps0 = 1; most iterations move


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_cut_invariance_and_determinism(la, dtype):
    import altlib
    Cn, p, W = 65, 8, 150
    model = model_of(la, p, dtype)
    q0 = cases.start(Cn, p)
    one = cases.warm(model, q0, W, seed=23)
    assert one["info"]["windows"] == 1
    for name, kw in (("1 + 7 + 142", dict(cuts=[1, 7, 142])), ("150 single calls", dict(cuts=[1] * W)), ("device pointers", dict(on_device=True)),
                     ("device pointers in pieces", dict(on_device=True, cuts=[1, 7, 142])), ("twice over", dict())):
        assert cases.same_bytes(one, cases.warm(model, q0, W, seed=23, **kw)) is None, name
    assert cases.same_bytes(one, cases.warm(model, q0, W, seed=24)) is not None
    altlib.install()  # the second build of the same sources
    try:
        X, y, ps = cases.data(p)
        m_alt = la.LogReg(X, y, ps, dtype=dtype)
        alt = cases.warm(m_alt, q0, W, seed=23)
        m_alt.close()
    finally:
        altlib.uninstall()
    assert cases.same_bytes(one, alt) is None


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_a_nan_start_touches_its_own_chain_and_coordinate_only(la, dtype):
    Cn, p, W, bad, j = 65, 8, 60, 5, 1
    model = model_of(la, p, dtype)
    q0 = cases.start(Cn, p)
    q0[bad, j] = np.nan
    res = cases.warm(model, q0, W, seed=29)
    assert np.all(res["astat"][:, bad] == 0.0) and np.all(np.isnan(res["out"][:, bad, j]))  # its abar contribution is 0
    others = np.delete(np.arange(Cn), bad)
    abar, tol = ar.abar_of(res["astat"])
    assert np.all(np.abs(res["trace"][:, 1] - abar) <= tol) and np.all(np.abs(res["trace"][:, 1] - res["astat"][:, others].sum(axis=1) / Cn) <= tol)
    var, dmm = res["metric"][0]
    assert not np.isfinite(var[j]) and dmm[j] == 1.0 and res["dmm"][j] == 1.0  # the coordinate's variance is non-finite, its dmm kept
    assert np.all(np.isfinite(np.delete(var, j))) and np.all(np.delete(res["dmm"], j) != 1.0)
    assert res["info"]["metric_skipped"] == 1 and res["info"]["windows"] == 1
    # The other chains of its wave (chains 4 .. 7) are what they are beside a finite neighbour.  The pooled step is teacher-forced: every
    # iteration is replayed through the plain kernel with this run's (eps_t, dmm_t) from this run's previous states, chain 5's NaN
    # replaced by a finite number -- a run of its own from a finite start would have another eps sequence.
    wave = slice(4, 8)

    def finite(prev):
        prev = prev.copy()
        prev[bad - 4, j] = 0.25
        return prev
    sub = {k: (v[:, wave] if k in ("out", "depth", "astat") else v) for k, v in res.items()}
    keep = [0, 2, 3]
    moved = replay(la, model, q0[wave], sub, W, seed=29, chain_offset=4, chains=keep, patch=finite)
    assert moved > W // 2


def test_one_chain_no_metric_and_chain_shards(la):
    p, W = 8, 150
    model = model_of(la, p, "float64")
    # C = 1: the window's n is its length, n - 1 = 24
    one = cases.warm(model, cases.start(1, p), W, seed=31)
    assert one["trace"][99, 4] == 25 and one["trace"][99, 3] == 0 and one["trace"][100, 3] == -1
    mt = ar.metric_of(one["out"][75:100], np.ones(p))
    assert np.all(np.abs(one["metric"][0, 0] - mt["var"]) <= mt["tol_var"]) and np.allclose(one["metric"][0, 0], np.var(one["out"][75:100, 0].astype(np.float64), axis=0, ddof=1), rtol=1e-10)
    # adapt_metric = False leaves dmm0
    d0 = np.linspace(0.5, 3.0, p)
    q0 = cases.start(9, p)
    fixed = cases.warm(model, q0, W, seed=31, dmm0=d0, adapt_metric=False)
    assert fixed["dmm"].tobytes() == d0.tobytes() and fixed["info"]["n_windows"] == 0 == fixed["info"]["windows"] and np.all(fixed["trace"][:, 3] == -1)
    assert replay(la, model, q0, dict(fixed, metric=np.zeros((0, 2, p))), W, seed=31, dmm0=d0) > W // 2
    tf = ar.teacher_forced(fixed["astat"], fixed["out"], W, d0, adapt_metric=False)
    assert np.max(np.abs(fixed["trace"][:, 0] - tf["eps"]) / tf["eps"]) <= cases.EPS_RTOL and abs(fixed["eps"] - tf["final"]) <= cases.EPS_RTOL * tf["final"]
    # shards at chain_offset 1, 2, 3 draw the streams of the global chain ids: iteration 0 (eps0 and dmm0: nothing pooled yet) is the
    # whole run's, and every later iteration is the plain kernel's at that offset with the shard's own (eps_t, dmm_t)
    whole = cases.warm(model, q0, 60, seed=37)
    for off in (1, 2, 3):
        sh = cases.warm(model, q0[off:off + 5], 60, seed=37, chain_offset=off)
        assert sh["out"][0].tobytes() == whole["out"][0][off:off + 5].tobytes() and sh["astat"][0].tobytes() == whole["astat"][0][off:off + 5].tobytes()
        assert sh["out"][1:].tobytes() != whole["out"][1:, off:off + 5].tobytes()  # a shard adapts by itself
        assert replay(la, model, q0[off:off + 5], sh, 60, seed=37, chain_offset=off) > 30


def test_it_works_on_pima_from_eps_1_and_the_unit_metric(la, pima, pscale, map_beta):
    """64 chains, W = 300, then 200 sampling iterations through mcmc(res.state, res.kernel).  The bands are sanity conditions from the CPU
    (tools/adapt_cpu_bands.py: adapt_reference.py driving the NumPy NUTS on the same model, 5 seeds; figures in profiles/r18_adapt.txt):
    2 x the reference's own spread around 1 for pre_j / var_golden_j, and around delta for the sampling run's mean acceptance statistic."""
    ref = load_golden("posterior_hmc.json")["pooled"]
    bands = load_golden("adapt_pima_bands.json")
    X, y = pima
    model = la.LogReg(X, y, pscale, dtype="float32")
    rng = np.random.default_rng(41)
    sd = np.array(ref["sd"])
    q0 = map_beta + 0.5 * sd * rng.standard_normal((64, 8))
    res = la.nuts_warmup(model.lpost, model.glp, q0, 300, seed=43)
    assert res.trace[0, 0] == 1.0 and res.info["windows"] == 3 and res.info["metric_skipped"] == 0 and res.kernel.params["eps"] == res.eps
    out, info = la.mcmc(res.state, res.kernel, thin=1, iters=200, verb=False, seed=47, return_info=True)
    summ = la.summarise(out)
    z = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    var_golden = sd ** 2
    ratio = res.pre / var_golden
    acc = float(np.mean(info["mean_accept_stat"]))
    print("PIMA eps %.4g pre %s ratio %s accept %.4f depth %.3f z %s divergent %d" % (res.eps, np.round(res.pre, 5), np.round(ratio, 3), acc, float(np.mean(info["mean_depth"])),
                                                                                    np.round(z, 2), int(info["divergent"].sum())))
    assert info["divergent"].sum() == 0
    assert np.max(np.abs(z)) < 3.0
    assert np.argmax(res.pre) == 0 and np.array_equal(np.argsort(res.pre), np.argsort(var_golden))  # the intercept's is the largest
    s = 2.0 * bands["ratio_spread"]
    assert np.all(np.abs(ratio - 1.0) <= s), (ratio, s)
    assert abs(acc - 0.8) <= 2.0 * bands["accept_spread"], (acc, bands["accept_spread"])
    model.close()
