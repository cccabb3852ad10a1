"""PSIS-LOO on the GPU (include/logreg_hip_loo.h, csrc/lr_loo.h) against tests/loo_reference.py, stage by stage.

Fill: `loglik()` of every case of loo_cases.FILL (both dtypes, real widths 3 ... 128, n in {1, 63, 257}, S in {1, 24, 255, 1000}, one
batch and uneven batches, host and device memory) against the float64 reference on the same dtype-rounded inputs.
PSIS: the table against the NumPy reference fed the DEVICE's own `loglik()` matrix, so the fill's error does not enter; n_tail and
the pattern of infinite k-hat must be identical, rows 0 - 3 meet the bound.

The bounds are measured, not chosen (profiles/r14_loo.txt; `python tests/test_gpu_loo.py --measure` prints the figures):
  fill, float64    8 x the largest deviation of the kernel's matrix from the float64 reference over the case list
  fill, float32    8 x the largest deviation of the REFERENCE's float32 mode from its float64 mode over the case list -- what any float32
                   evaluation of the formulae costs; the kernel's own deviation is printed beside it
  PSIS             8 x the largest deviation of the kernel's table from the reference over every table this file compares (the
                   model cases of both dtypes and the hand-made matrices), per row: elpd, khat, n_eff / S, lppd
8 x is the repository's convention (profiles/r8_nuts_reference.txt).
"""
import faulthandler
import sys

import numpy as np
import pytest

import loo_cases as lc
import loo_reference as lref
import predict_cases as pc

pytestmark = pytest.mark.gpu

# measured figures (profiles/r14_loo.txt) -> bounds = 8 x
MEASURED = {
    "fill": {"float64": 1.332e-15, "float32": 6.623e-06},  # float64: the kernel against the reference; float32: the reference's float32 mode against its float64 mode
    "psis": {"elpd": 1.954e-14, "khat": 8.171e-13, "n_eff": 3.553e-15, "lppd": 4.441e-16},
}
BOUND = {k: {q: 8.0 * v for q, v in d.items()} for k, d in MEASURED.items()}
PSIS_ROWS = ("elpd", "khat", "n_eff", "lppd")
_REF = {}


@pytest.fixture(autouse=True)
def step_timeout():
    """Every step under its own time limit: a step that hangs ends the whole run (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def la():
    import logreg_amd as la
    return la


def fill_reference(name, dtype):
    key = (name, dtype)
    if key not in _REF:
        _REF[key] = lref.loglik_matrix(*lc.rounded(lc.fill_case(name), np.dtype(dtype).type))
    return _REF[key]


def run_fill(la, case, dtype, how, want_table=False):
    model = la.LogReg(case["X"], case["y"], case["pscale"], dtype=dtype)
    acc = la.PsisLoo(model, case["B"].shape[0])
    B = case["B"].astype(model.np_dtype)
    pc.feed(la, acc, B, how)
    assert acc.n_draws == B.shape[0]
    ll = acc.loglik()
    assert ll.dtype == model.np_dtype and ll.shape == (B.shape[0], model.n)
    t = acc.table() if want_table else None
    acc.close()
    model.close()
    return (ll, t) if want_table else ll


def psis_deviations(t, ref, S):
    """Per row of PSIS_ROWS the largest |difference| (n_eff divided by S); n_tail, the infinities of khat and every NaN must agree
    exactly, else the figure is infinite."""
    t, ref = np.asarray(t), np.asarray(ref)
    ok = np.array_equal(t[4], ref[4], equal_nan=True) and np.array_equal(np.isinf(t[1]), np.isinf(ref[1])) and np.array_equal(np.isnan(t), np.isnan(ref))
    out = {}
    for k, name in enumerate(PSIS_ROWS):
        same = (t[k] == ref[k]) | (np.isnan(t[k]) & np.isnan(ref[k]))
        with np.errstate(invalid="ignore"):
            d = np.where(same, 0.0, np.abs(t[k] - ref[k]))
        d = float(np.where(np.isnan(d), np.inf, d).max()) / (S if name == "n_eff" else 1.0)
        out[name] = d if ok else np.inf
    return out


def check_psis(label, t, ref, S):
    assert np.array_equal(t[4], ref[4], equal_nan=True), (label, "n_tail", t[4], ref[4])
    assert np.array_equal(np.isinf(t[1]), np.isinf(ref[1])), (label, "the pattern of khat == inf")
    assert np.array_equal(np.isnan(t), np.isnan(ref)), (label, "NaN pattern")
    d = psis_deviations(t, ref, S)
    print(f"[loo] psis {label}: " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()) + "   bounds " + "  ".join(f"{BOUND['psis'][k]:.3e}" for k in PSIS_ROWS))
    for k in PSIS_ROWS:
        assert d[k] <= BOUND["psis"][k], (label, k, d[k], BOUND["psis"][k])
    return d


# ---- 1. the fill stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", lc.FILL_NAMES)
def test_loglik_against_the_reference_and_batchings_give_identical_bytes(la, name, dtype):
    case = lc.fill_case(name)
    ref = fill_reference(name, dtype)
    got = []
    for how in case["batchings"]:
        ll = run_fill(la, case, dtype, how)
        assert np.all(np.isfinite(ll)) and np.all(ll <= 0)
        d = float(np.max(np.abs(ll.astype(np.float64) - ref)))
        print(f"[loo] fill {name} {dtype} {how}: {d:.3e}   bound {BOUND['fill'][dtype]:.3e}")
        assert d <= BOUND["fill"][dtype], (name, dtype, how, d, BOUND["fill"][dtype])
        got.append(ll)
    assert got[0].tobytes() == got[1].tobytes(), (name, dtype)  # per-pair arithmetic: how the draws were cut cannot matter


# ---- 2. the PSIS stage ------------------------------------------------------------------------------------------------------------------
def run_model_case(la, name, dtype):
    case = lc.model_case(name)
    model = la.LogReg(case["X"], case["y"], case["pscale"], dtype=dtype)
    acc = la.PsisLoo(model, case["B"].shape[0]).update(case["B"])
    ll, t = acc.loglik(), acc.table()
    res = acc.result()
    acc.close()
    model.close()
    return ll, t, res


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", lc.PSIS_NAMES)
def test_table_against_the_reference_on_the_devices_own_matrix(la, name, dtype):
    ll, t, res = run_model_case(la, name, dtype)
    S = ll.shape[0]
    ref = lref.psis_table(ll)
    check_psis(f"{name} {dtype}", t, ref, S)
    assert res["n_draws"] == S and res["n_khat_over_0_7"] == int(np.sum(ref[1] > 0.7))
    assert abs(res["elpd_loo"] - ref[0].sum()) <= BOUND["psis"]["elpd"] * ll.shape[1]
    assert abs(res["p_loo"] - (ref[3] - ref[0]).sum()) <= (BOUND["psis"]["elpd"] + BOUND["psis"]["lppd"]) * ll.shape[1]
    if dtype == "float64":  # what the case list is for (asserted on the reference side; tests/test_loo_cpu.py has the whole span)
        k = ref[1]
        if name == "pima_S25":
            assert np.any(k < 0) and np.sum(k > 0.7) > 0 and np.any((k > 1) & np.isfinite(k))
        if name == "synthetic_n60_p32_S4096":
            assert np.any((k > 1) & np.isfinite(k)) and np.sum(k > 0.7) > 0
        if name == "synthetic_n300_p3_S4096":
            assert np.sum(k > 0.7) == 0 and np.any(k < 0)


# ---- 3. hand-made matrices through psis_from_loglik ----------------------------------------------------------------------------------------
def hand_made():
    """name -> [S, r] matrix; every one is compared with the reference (and belongs to the measured set)"""
    rng = np.random.default_rng(2024)
    out = {}
    out["constant_S100"] = np.column_stack([np.full(100, -0.7), -rng.exponential(size=100)])
    out["raw_S24"] = -rng.exponential(size=(24, 3))
    out["smoothed_S25"] = -rng.exponential(size=(25, 3))
    t100 = -rng.exponential(size=(100, 2)) * 3.0  # M = 20
    o = np.argsort(t100[:, 0])
    t100[o[12:25], 0] = t100[o[20], 0]  # the cutoff value reaches into the would-be tail: n_t = 12
    o = np.argsort(t100[:, 1])
    t100[o[3:40], 1] = t100[o[20], 1]   # ... n_t = 3: raw weights
    out["ties_S100"] = t100
    k = np.arange(1000, dtype=np.float64)
    out["last_digit_f64_S1000"] = np.column_stack([-(1.0 + rng.permutation(k) * 2.0 ** -52), -(1.0 + (k % 7) * 2.0 ** -52)])
    out["last_digit_f32_S1000"] = np.column_stack([-(1.0 + rng.permutation(k) * 2.0 ** -23), -(1.0 + (k % 7) * 2.0 ** -23)]).astype(np.float32)
    out["wide_span_S2000"] = np.column_stack([rng.permutation(-np.logspace(-300, np.log10(700.0), 2000)), -np.logspace(-300, np.log10(700.0), 2000)])
    out["mixed_sign_S500"] = rng.standard_normal((500, 2)) * 2.0  # log densities may be positive: the keys' top bit differs
    return out


@pytest.mark.parametrize("name", ["constant_S100", "raw_S24", "smoothed_S25", "ties_S100", "last_digit_f64_S1000", "last_digit_f32_S1000", "wide_span_S2000",
                                  "mixed_sign_S500"])
def test_hand_made_matrices(la, name):
    L = hand_made()[name]
    t = la.psis_from_loglik(L)
    ref = lref.psis_table(L)
    S = L.shape[0]
    check_psis(name, t, ref, S)
    if name == "constant_S100":
        assert t[4, 0] == 0 and t[1, 0] == np.inf and t[0, 0] == -0.7  # elpd = l exactly; lppd is held to its bound above
    if name == "raw_S24":
        assert np.all(t[4] == 4) and np.all(t[1] == np.inf)
    if name == "smoothed_S25":
        assert np.all(t[4] == 5) and np.all(np.isfinite(t[1]))
    if name == "ties_S100":
        assert t[4, 0] == 12 and np.isfinite(t[1, 0]) and t[4, 1] == 3 and t[1, 1] == np.inf
    if name.startswith("last_digit"):
        assert t[4, 0] == lref.tail_length(S)  # distinct values one unit in the last place apart: the selection is exact
    if name == "wide_span_S2000":
        assert t[4, 0] == t[4, 1] == ref[4, 0] > 0  # (most of the column rounds to v = -700: ties at the cutoff)
    d = la.DeviceArray.from_host(0, L)  # from device memory: the same bytes
    assert la.psis_from_loglik(d).tobytes() == t.tobytes()
    d.free()


def test_two_to_the_twenty_draws_and_one_past_the_cap(la):
    from logreg_amd import _lib
    S = _lib.LOO_MAX_DRAWS
    rng = np.random.default_rng(7)
    L = np.column_stack([-rng.exponential(size=S), -np.abs(rng.standard_t(3, size=S)) * 2.0])
    t = la.psis_from_loglik(L)
    ref = lref.psis_table(L)
    assert np.all(ref[4] == 3072)
    check_psis("S = 2^20", t, ref, S)
    assert la.psis_from_loglik(L).tobytes() == t.tobytes()
    with pytest.raises(la.LogregHipError, match=r"error -3: .*LR_LOO_MAX_DRAWS"):  # LR_ERR_UNSUPPORTED, with the reason
        la.psis_from_loglik(np.zeros((S + 1, 1), dtype=np.float32))


def test_one_nan_entry_makes_its_row_nan_and_leaves_the_neighbour_alone(la, pima, pscale):
    rng = np.random.default_rng(11)
    L = -rng.exponential(size=(700, 3))
    clean = la.psis_from_loglik(L)
    bad = L.copy()
    bad[123, 1] = np.nan
    t = la.psis_from_loglik(bad)
    assert np.all(np.isnan(t[:, 1])) and np.all(np.isfinite(clean))
    assert t[:, [0, 2]].tobytes() == clean[:, [0, 2]].tobytes()
    check_psis("nan entry", t, lref.psis_table(bad), 700)
    # through a model, a NaN coordinate in one draw reaches every row
    X, y = pima
    model = la.LogReg(X, y, pscale, dtype="float64")
    B = lc.model_case("pima_S255")["B"].copy()
    acc = la.PsisLoo(model, 600).update(B)
    assert np.all(np.isfinite(acc.table()[[0, 2, 3, 4]]))
    B[17, 3] = np.nan
    acc.reset()
    assert acc.n_draws == 0 and np.all(np.isnan(acc.table()))  # empty: NaN by definition
    acc.update(B)
    assert np.all(np.isnan(acc.table())) and np.all(np.isnan(acc.loglik()[17])) and np.all(np.isfinite(acc.loglik()[16]))
    with pytest.raises(ValueError, match="exceed max_draws"):
        acc.update(np.zeros((346, 8)))
    with pytest.raises(la.LogregHipError, match="exceed max_draws"):  # the library refuses it too, and stays as it was
        _raw_accumulate(acc, np.zeros((346, 8)))
    assert acc.n_draws == 255 and acc.loglik().shape == (255, 200)
    acc.close()
    from logreg_amd import _lib
    with pytest.raises(la.LogregHipError, match=r"error -3: .*LR_LOO_MAX_DRAWS"):  # the accumulator states the same cap
        la.PsisLoo(model, _lib.LOO_MAX_DRAWS + 1)
    model.close()


def _raw_accumulate(acc, draws):
    from logreg_amd import _lib
    a = np.ascontiguousarray(draws, dtype=acc.model.np_dtype)
    _lib.check(acc._L.lr_loo_accumulate(acc.handle, a.ctypes.data, a.shape[0], 0, None))


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_same_calls_same_bytes_and_both_builds_agree(la, dtype):
    """The same call sequence twice gives identical bytes; the production library and the second build (tests/altlib.py: default
    scheduler, SLP on) give identical bytes -- every sum runs over a fixed tree with spelled-out fma."""
    from logreg_amd import _lib
    import altlib
    hm = hand_made()["ties_S100"].astype(dtype)
    for name in lc.DETERMINISM_NAMES:
        case = lc.fill_case(name)
        how = case["batchings"][1]
        a = run_fill(la, case, dtype, how, want_table=True)
        b = run_fill(la, case, dtype, how, want_table=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
        pa = la.psis_from_loglik(hm)
        L = altlib.install()
        try:
            _lib.bind_loo(L)
            assert _lib.load() is L
            c = run_fill(la, case, dtype, how, want_table=True)
            pcalt = la.psis_from_loglik(hm)
        finally:
            altlib.uninstall()
            _lib.bind_loo(_lib.load())
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes(), name
        assert pa.tobytes() == pcalt.tobytes()


def test_both_builds_agree_on_a_model_case_with_long_tails(la):
    from logreg_amd import _lib
    import altlib
    a = run_model_case(la, "synthetic_n60_p32_S4096", "float64")
    L = altlib.install()
    try:
        _lib.bind_loo(L)
        c = run_model_case(la, "synthetic_n60_p32_S4096", "float64")
    finally:
        altlib.uninstall()
        _lib.bind_loo(_lib.load())
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


# ---- 5. mcmc(..., loo=acc) -------------------------------------------------------------------------------------------------------------------
def mcmc_runs(la, dtype):
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
    acc = la.PsisLoo(model, C * iters)
    with_loo = la.mcmc(init, kern, summary_only=True, loo=acc, **kw)
    mat, info = la.mcmc(init, kern, return_info=True, **kw)
    acc2 = la.PsisLoo(model, C * iters)
    mat2, info2 = la.mcmc(init, kern, return_info=True, loo=acc2, **kw)
    acc3 = la.PsisLoo(model, C * iters).update(mat)  # the kept draws of the same seeded run, by hand
    small = la.PsisLoo(model, C * iters - 1)
    return dict(model=model, kern=kern, init=init, kw=kw, plain=plain, with_loo=with_loo, acc=acc, acc2=acc2, acc3=acc3, small=small, mat=mat, mat2=mat2,
                info=info, info2=info2, S=C * iters)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype):
    r = mcmc_runs(la, dtype)
    plain, with_loo, acc, acc2, acc3, S = r["plain"], r["with_loo"], r["acc"], r["acc2"], r["acc3"], r["S"]
    assert acc.n_draws == acc2.n_draws == acc3.n_draws == S
    assert set(with_loo) == set(plain) | {"loo"} and set(r["info2"]) == set(r["info"]) | {"loo"}
    for key in plain:  # state, statistics, accept rate, plan: exactly the run without `loo`
        a, b = plain[key], with_loo[key]
        assert (np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) if not isinstance(a, dict) else a == b), key
    assert r["mat"].tobytes() == r["mat2"].tobytes()
    assert np.array_equal(r["info"]["accepts"], r["info2"]["accepts"]) and np.array_equal(r["info"]["state"], r["info2"]["state"])
    assert np.array_equal(r["info"]["state"], plain["state"])
    t = acc.table()
    assert t.tobytes() == acc2.table().tobytes() == acc3.table().tobytes()  # chunk by chunk on the device = the kept draws by hand
    assert acc.loglik().tobytes() == acc3.loglik().tobytes()
    res = with_loo["loo"]
    assert res["n_draws"] == S and np.array_equal(res["elpd_i"], t[0]) and res["elpd_i"].shape == (200,)
    assert np.isfinite(res["elpd_loo"]) and 0 < res["p_loo"] < 20 and res["se"] > 0 and res["looic"] == -2 * res["elpd_loo"]
    check_psis(f"mcmc {dtype}", t, lref.psis_table(acc.loglik()), S)
    # too small a max_draws is refused before the first launch: nothing was appended, no chain was made
    with pytest.raises(ValueError, match="max_draws"):
        la.mcmc(r["init"], r["kern"], summary_only=True, loo=r["small"], **r["kw"])
    assert r["small"].n_draws == 0
    with pytest.raises(ValueError, match="max_draws"):  # a second run into a full accumulator
        la.mcmc(r["init"], r["kern"], summary_only=True, loo=acc, **r["kw"])
    one = la.psis_loo(r["model"], r["mat"])
    assert one["elpd_i"].tobytes() == t[0].tobytes()
    for q in (acc, acc2, acc3, r["small"]):
        q.close()
    r["model"].close()


def test_host_draws_one_longer_than_a_staging_piece_give_the_bytes_of_two_updates(la):
    """The one path no case above reaches: host draws that do not fit one staging piece, padded to the kernel width on the way.  One
    `update` with a draw more than a piece is the launch sequence of two `update`s cut at the piece boundary, so the bytes are the same."""
    # draws are staged in pieces of max(1024, 256 MB / (P esize)) draws, P the padded width: p = 100 -> P = 128, 256 MB / (128 x 8 bytes) =
    # 262144 draws.  (A change of the 256 MB needs another shape here.)
    p, piece = 100, 262144
    rng = np.random.default_rng(14)
    X = rng.standard_normal((16, p))
    y = (rng.random(16) < 0.5).astype(np.float64)
    B = 0.05 * rng.standard_normal((piece + 1, p))
    model = la.LogReg(X, y, np.full(p, 2.0), dtype="float64")
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        acc = la.PsisLoo(model, piece + 1)
        s0 = 0
        for S in cuts:
            acc.update(B[s0:s0 + S])
            s0 += S
        assert acc.n_draws == piece + 1
        out.append((acc.loglik(), acc.table()))
        acc.close()
    model.close()
    assert np.all(np.isfinite(out[0][0])) and np.all(out[0][0] < 0) and np.all(np.isfinite(out[0][1][[0, 2, 3, 4]]))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def measure():
    """Print the figures of profiles/r14_loo.txt: the fill's largest deviation per dtype (kernel against the float64 reference; the
    reference's float32 mode against its float64 mode) and the PSIS stage's per row over every table this file compares."""
    import logreg_amd as la
    fig = {("fill", "kernel", "float64"): 0.0, ("fill", "kernel", "float32"): 0.0, ("fill", "ref32", "float32"): 0.0}
    fig.update({("psis", k): 0.0 for k in PSIS_ROWS})
    for name in lc.FILL_NAMES:
        case = lc.fill_case(name)
        for dtype in ("float64", "float32"):
            ref = fill_reference(name, dtype)
            for how in case["batchings"]:
                d = float(np.max(np.abs(run_fill(la, case, dtype, how).astype(np.float64) - ref)))
                print(f"fill kernel {dtype} {name} {how}: {d:.3e}", flush=True)
                fig[("fill", "kernel", dtype)] = max(fig[("fill", "kernel", dtype)], d)
        X32, y, B32 = lc.rounded(case, np.float32)
        d = float(np.max(np.abs(lref.loglik_matrix(X32, y, B32, mode="float32").astype(np.float64) - fill_reference(name, "float32"))))
        print(f"fill reference float32 mode vs float64 mode {name}: {d:.3e}", flush=True)
        fig[("fill", "ref32", "float32")] = max(fig[("fill", "ref32", "float32")], d)

    def fold(label, t, ref, S):
        d = psis_deviations(t, ref, S)
        print(f"psis {label}: " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()), flush=True)
        for k in PSIS_ROWS:
            fig[("psis", k)] = max(fig[("psis", k)], d[k])
    for name in lc.PSIS_NAMES:
        for dtype in ("float64", "float32"):
            ll, t, _ = run_model_case(la, name, dtype)
            ref = lref.psis_table(ll)
            fold(f"{name} {dtype} (khat {np.nanmin(ref[1]):.3f} .. {np.max(ref[1][np.isfinite(ref[1])]):.3f}, {int(np.sum(ref[1] > 0.7))} over 0.7)", t, ref, ll.shape[0])
    for name, L in hand_made().items():
        fold(name, la.psis_from_loglik(L), lref.psis_table(L), L.shape[0])
    rng = np.random.default_rng(7)
    S = 1 << 20
    L = np.column_stack([-rng.exponential(size=S), -np.abs(rng.standard_t(3, size=S)) * 2.0])
    fold("S = 2^20", la.psis_from_loglik(L), lref.psis_table(L), S)
    rng = np.random.default_rng(11)
    L = -rng.exponential(size=(700, 3))
    fold("nan entry (clean)", la.psis_from_loglik(L), lref.psis_table(L), 700)
    for dtype in ("float64", "float32"):
        r = mcmc_runs(la, dtype)
        fold(f"mcmc {dtype}", r["acc"].table(), lref.psis_table(r["acc"].loglik()), r["S"])
    for k, v in fig.items():
        print("FIGURE", *k, f"{v:.3e}")


if __name__ == "__main__":
    import os
    if sys.argv[1:] != ["--measure"]:
        sys.exit("usage: python tests/test_gpu_loo.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
