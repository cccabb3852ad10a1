"""The draw-consuming kernels at saturated logits (cases: tests/predict_regime_cases.py; reference and bounds: tests/pair_reference.py;
both are checked without a GPU by tests/test_predict_regimes_cpu.py).

k_predict_partial (predictive probability, lppd, WAIC) and k_loo_fill (the pointwise log-likelihood matrix k_psis reads) go through one
device function, pred_pair of csrc/lr_predict.h, with its own code for what happens when |t| = |x . beta| is large: a select-clamp at -750
in float64, the hardware exponential fed -|t| log2(e) unclamped in float32, pred_rcp, and sigma(-|t|) formed as e r.  The posterior-like
draws of tests/test_gpu_predict.py and tests/test_gpu_loo.py never leave the tame regime, and their bounds are absolute; here every case
walks |t| from 1 to 5000 in one launch, and sets of nine draws in which every row is confidently wrong hold the mean of L -- whose
logarithm is lppd -- to a RELATIVE bound.

  PosteriorPredictive.table()   every entry within the table bounds; row 2 also in its logarithm where the reference clears its bound;
                                no NaN, 0 <= pi <= 1, 0 <= mean L <= 1, mean l <= 0 and finite, rows 1 and 4 >= 0; two batchings that cut
                                the draws alike give identical bytes
  lppd(), waic()                -inf exactly where row 2 is 0, finite elsewhere, never NaN; waic()'s sums follow, p_waic is finite, and se is
                                NaN exactly for one row or a zero in row 2 (check_lppd_and_waic states the rule)
  PsisLoo.loglik()              every element within tol_l, finite and <= 0; the two batchings give identical bytes
  PsisLoo.table()               against loo_reference.psis_table on the device's own matrix: n_tail, the pattern of khat = inf, the NaN
                                pattern and the places of lppd = -inf identical; rows 0 - 3 within tests/test_gpu_loo.py's BOUND["psis"]
                                plus 4 2^-53 |ref| on elpd and lppd (their final subtraction of a = max -l rounds at a magnitude of
                                thousands, which the tame cases that bound was measured on never had)
  a NaN coordinate              in one draw of the mixed set: the whole table NaN; in the matrix that draw's row NaN, every other row unchanged

Nothing here is fitted to the kernels: every bound comes from the inputs.  `python tests/test_gpu_predict_regimes.py --measure` prints
the largest error / bound per table row, case and dtype and the smallest nonzero L the device returns (profiles/r25_predict_regimes.txt).
"""
import faulthandler
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_reference as lref  # noqa: E402
import pair_reference as pref  # noqa: E402
import predict_cases as pc  # noqa: E402
import predict_regime_cases as rc  # noqa: E402
from test_gpu_loo import BOUND as LOO_BOUND, PSIS_ROWS  # noqa: E402

pytestmark = pytest.mark.gpu
CASE_DTYPE = [(n, d) for n in rc.NAMES for d in rc.DTYPES]
RATIOS = {}


@pytest.fixture(autouse=True)
def step_timeout():
    """Every test under its own time limit: one that hangs ends the whole run (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def la():
    import logreg_amd as la
    yield la
    print("\nlargest error / bound per case and dtype")
    for key in sorted(RATIOS):
        print("  %-18s %-8s " % key + "  ".join(f"{k} {v:.3f}" for k, v in RATIOS[key].items()))


def stop_on_hip_error(e):
    """A HIP runtime error (LR_ERR_HIP, -2) ends the whole run: nothing more is started on a device that has faulted."""
    if "error -2" in str(e):
        pytest.exit("HIP runtime error: " + str(e), returncode=3)


def note(name, dtype, key, value):
    have = RATIOS.setdefault((name, dtype), {})
    have[key] = max(have.get(key, 0.0), value)


def check_table(name, dtype, which, t, R, bad):
    """One table against the reference; failures are appended to `bad`, ratios noted."""
    ref, tol = R["table"], R["ttol"]
    labelled = R["ref"]["labels"]
    if not np.array_equal(np.isnan(t), np.isnan(ref)):
        bad.append((which, "NaN pattern", np.argwhere(np.isnan(t) != np.isnan(ref))[:4].tolist()))
        return
    rows = range(5) if labelled else range(2)
    for k in rows:
        q = pref.ratio(t[k], ref[k], tol[k])
        note(name, dtype, f"row{k}", q)
        if not q <= 1.0:
            with np.errstate(divide="ignore", invalid="ignore"):
                i = int(np.nanargmax(np.abs(t[k] - ref[k]) / tol[k]))
            bad.append((which, f"row {k}", round(q, 3), "row index %d" % i, float(t[k, i]), float(ref[k, i]), float(tol[k, i])))
    # hard facts, whatever the bounds
    if not (np.all(t[0] >= 0) and np.all(t[0] <= 1)):
        bad.append((which, "pi outside [0, 1]", float(t[0].min()), float(t[0].max())))
    if not np.all(t[1] >= 0):
        bad.append((which, "row 1 < 0", float(t[1].min())))
    if labelled:
        if not (np.all(t[2] >= 0) and np.all(t[2] <= 1)):
            bad.append((which, "mean L outside [0, 1]", float(t[2].min()), float(t[2].max())))
        if not (np.all(np.isfinite(t[3])) and np.all(t[3] <= 0)):
            bad.append((which, "mean l > 0 or not finite", float(t[3].max())))
        if not np.all(t[4] >= 0):
            bad.append((which, "row 4 < 0", float(t[4].min())))
        # row 2 in its logarithm: lppd
        clear = ref[2] - tol[2] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            dlog = np.abs(np.log(t[2]) - np.log(ref[2]))
            q = np.where(clear, dlog / (tol[2] / (ref[2] - tol[2])), 0.0)
        q = np.where(np.isnan(q), np.inf, q)
        note(name, dtype, "log row2", float(q.max()))
        if not np.all(q <= 1.0):
            i = int(np.argmax(q))
            bad.append((which, "log row 2", float(q[i]), "row index %d" % i, float(t[2, i]), float(ref[2, i])))
        if not np.all(t[2][~clear] <= (ref[2] + tol[2])[~clear]):
            bad.append((which, "row 2 above ref + tol where the reference does not clear its bound"))


def check_lppd_and_waic(which, t, lppd, waic, bad):
    """lppd() and waic() of a table t: never NaN where a number is defined.  With zero = (row 2 == 0):
        lppd_i, elpd_i      -inf exactly where zero, finite elsewhere        p_waic_i, p_waic      finite (row 4 is)
        lppd, elpd_waic     -inf if any zero, else finite                    waic = -2 elpd_waic   +inf if any zero, else finite
        se = sqrt(r var(elpd_i, ddof = 1))   NaN exactly when r == 1 (no variance of one number) or any zero (the variance of a set
                                             that holds -inf is inf - inf), finite otherwise"""
    zero = t[2] == 0
    r, any_zero = t.shape[1], bool(np.any(zero))
    for key, v in (("lppd()", lppd), ("lppd_i", waic["lppd_i"]), ("elpd_i", waic["elpd_i"])):
        if np.any(np.isnan(v)) or not np.array_equal(v == -np.inf, zero) or not np.all(np.isfinite(v[~zero])):
            bad.append((which, key, np.asarray(v)[:8].tolist()))
    if not np.all(np.isfinite(waic["p_waic_i"])) or not np.isfinite(waic["p_waic"]):
        bad.append((which, "p_waic", waic["p_waic"]))
    for key, want in (("lppd", -np.inf), ("elpd_waic", -np.inf), ("waic", np.inf)):
        if not (waic[key] == want if any_zero else np.isfinite(waic[key])):
            bad.append((which, key, waic[key]))
    if not (np.isnan(waic["se"]) if r == 1 or any_zero else np.isfinite(waic["se"])):
        bad.append((which, "se", waic["se"], "r = %d, zeros in row 2: %s" % (r, any_zero)))


def check_psis(name, dtype, which, t, ref, S, bad):
    """PsisLoo.table() t against the reference's table of the device's own matrix: the patterns identical, rows 0 - 3 within the bounds of the
    module docstring; failures are appended to `bad`, ratios noted (the test and the measure mode share this)."""
    if not np.array_equal(t[4], ref[4]):
        bad.append((which, "n_tail", t[4][t[4] != ref[4]][:4].tolist(), ref[4][t[4] != ref[4]][:4].tolist()))
    if not np.array_equal(np.isinf(t[1]), np.isinf(ref[1])):
        bad.append((which, "the pattern of khat = inf", np.flatnonzero(np.isinf(t[1]) != np.isinf(ref[1]))[:4].tolist()))
    if not np.array_equal(np.isnan(t), np.isnan(ref)):
        bad.append((which, "NaN pattern", np.argwhere(np.isnan(t) != np.isnan(ref))[:4].tolist()))
    if not np.array_equal(t[3] == -np.inf, ref[3] == -np.inf):
        bad.append((which, "the places of lppd = -inf"))
    for k, row in enumerate(PSIS_ROWS):
        same = (t[k] == ref[k]) | (np.isnan(t[k]) & np.isnan(ref[k]))
        with np.errstate(invalid="ignore"):
            d = np.where(same, 0.0, np.abs(t[k] - ref[k])) / (S if row == "n_eff" else 1.0)
            bound = LOO_BOUND["psis"][row] + (4 * 2.0 ** -53 * np.abs(np.where(same, 0.0, ref[k])) if row in ("elpd", "lppd") else 0.0)
            qk = np.where(same, 0.0, d / bound)
        qk = np.where(np.isnan(qk), np.inf, qk)
        note(name, dtype, "psis " + row, float(qk.max()))
        if not np.all(qk <= 1.0):
            i = int(np.argmax(qk))
            bad.append((which, "psis " + row, float(qk[i]), "row index %d" % i, float(t[k, i]), float(ref[k, i])))


def run_predict(la, model, c, which, how):
    pp = la.PosteriorPredictive(model, c["X_new"], c["y_new"])
    try:
        B = c["sets"][which].astype(model.np_dtype)
        pc.feed(la, pp, B, how)
        assert pp.n_draws == B.shape[0]
        t = pp.table()
        if not pp.has_labels:
            return t, None, None
        with np.errstate(divide="ignore", invalid="ignore"):  # (log 0 = -inf is the answer asked for; check_lppd_and_waic holds the rest to its rule)
            return t, pp.lppd(), pp.waic()
    except la.LogregHipError as e:
        stop_on_hip_error(e)
        raise
    finally:
        pp.close()


def run_fill(la, model, c, which, how):
    B = c["sets"][which].astype(model.np_dtype)
    acc = la.PsisLoo(model, B.shape[0])
    try:
        pc.feed(la, acc, B, how)
        assert acc.n_draws == B.shape[0]
        return acc.loglik(), acc.table()
    except la.LogregHipError as e:
        stop_on_hip_error(e)
        raise
    finally:
        acc.close()


@pytest.mark.parametrize("name,dtype", CASE_DTYPE)
def test_predictive_table_lppd_and_waic(la, name, dtype):
    c = rc.case(name)
    model = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
    bad = []
    try:
        for which in rc.SETS:
            R = rc.reference(name, dtype, which)
            got = [run_predict(la, model, c, which, how) for how in c["batchings"]]
            t, lppd, waic = got[0]
            check_table(name, dtype, which, t, R, bad)
            if got[0][0].tobytes() != got[1][0].tobytes():
                bad.append((which, "the two batchings differ", np.argwhere(~((got[0][0] == got[1][0]) | np.isnan(got[0][0])))[:4].tolist()))
            if c["labels"] is None:
                assert lppd is None and np.all(np.isnan(t[2:]))
                continue
            check_lppd_and_waic(which, t, lppd, waic, bad)
    finally:
        model.close()
    print(name, dtype, "predict:", {k: round(v, 3) for k, v in RATIOS.get((name, dtype), {}).items()})
    assert not bad, bad


@pytest.mark.parametrize("name,dtype", CASE_DTYPE)
def test_loglik_matrix_and_psis_table(la, name, dtype):
    c = rc.case(name)
    model = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
    bad = []
    try:
        for which in rc.SETS:
            R = rc.reference(name, dtype, which, rows="model")
            got = [run_fill(la, model, c, which, how) for how in c["batchings"]]
            ll, t = got[0]
            S = ll.shape[0]
            assert ll.dtype == model.np_dtype and ll.shape == R["ref"]["l"].shape
            if not (np.all(np.isfinite(ll)) and np.all(ll <= 0)):
                bad.append((which, "loglik not finite or > 0", np.argwhere(~(np.isfinite(ll) & (ll <= 0)))[:4].tolist()))
                continue
            q = pref.ratio(ll, R["ref"]["l"], R["tol"]["l"])
            note(name, dtype, "fill l", q)
            if not q <= 1.0:
                s, i = np.unravel_index(int(np.argmax(np.abs(ll.astype(np.float64) - R["ref"]["l"]) / R["tol"]["l"])), ll.shape)
                bad.append((which, "loglik", round(q, 3), "draw %d row %d" % (s, i), float(ll[s, i]), float(R["ref"]["l"][s, i]), float(R["tol"]["l"][s, i])))
            if got[0][0].tobytes() != got[1][0].tobytes() or got[0][1].tobytes() != got[1][1].tobytes():
                bad.append((which, "the two batchings differ"))
            check_psis(name, dtype, which, t, lref.psis_table(ll), S, bad)
    finally:
        model.close()
    print(name, dtype, "loo:", {k: round(v, 3) for k, v in RATIOS.get((name, dtype), {}).items() if k.startswith(("fill", "psis"))})
    assert not bad, bad


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("name", ["p3_n37_plain", "p32_n257_plain", "p128_n130_plain"])
def test_a_nan_coordinate_among_saturated_draws(la, name, dtype):
    """The header's rule for non-finite input, where the draws around the NaN sit on every clamp: the whole table is NaN, never a finite wrong
    number (a clamp that drops a NaN -- fmax for the select -- answers L = 0, l = 0 there), and in the log-likelihood matrix the NaN draw's
    row is NaN and every other row keeps its bytes."""
    c = rc.case(name)
    model = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
    B = c["sets"]["mixed"].astype(model.np_dtype)
    bad_draw = 77  # in the second slice of both kernels, among draws at T = 5000
    nan = B.copy()
    nan[bad_draw, c["p"] - 1] = np.nan
    try:
        pp = la.PosteriorPredictive(model).update(nan)
        t = pp.table()
        pp.close()
        clean = la.PsisLoo(model, len(B)).update(B)
        acc = la.PsisLoo(model, len(B)).update(nan)
        ll0, ll, pt = clean.loglik(), acc.loglik(), acc.table()
        clean.close()
        acc.close()
    except la.LogregHipError as e:
        stop_on_hip_error(e)
        raise
    finally:
        model.close()
    assert np.all(np.isnan(t)), np.argwhere(~np.isnan(t))[:4].tolist()
    assert np.all(np.isnan(ll[bad_draw])) and np.all(np.isnan(pt))
    keep = np.arange(len(B)) != bad_draw
    assert ll[keep].tobytes() == ll0[keep].tobytes()


def measure():
    """Print the figures of profiles/r25_predict_regimes.txt: the largest error / bound per table row, case and dtype (and of the fill and
    the PSIS rows), and per dtype the smallest nonzero L the device returns (row 2 of single draws of the rungs) with the |t| it belongs to."""
    import logreg_amd as la
    smallest = {d: (np.inf, None, None) for d in rc.DTYPES}
    largest_zero = {d: 0.0 for d in rc.DTYPES}
    for name, dtype in CASE_DTYPE:
        c = rc.case(name)
        model = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
        for which in rc.SETS:
            bad = []
            check_table(name, dtype, which, run_predict(la, model, c, which, c["batchings"][0])[0], rc.reference(name, dtype, which), bad)
            R = rc.reference(name, dtype, which, rows="model")
            ll, t = run_fill(la, model, c, which, c["batchings"][0])
            note(name, dtype, "fill l", pref.ratio(ll, R["ref"]["l"], R["tol"]["l"]))
            check_psis(name, dtype, which, t, lref.psis_table(ll), ll.shape[0], bad)
            if bad:
                print("OUTSIDE", name, dtype, which, bad, flush=True)
            if c["labels"] is not None and which != "mixed":
                pp = la.PosteriorPredictive(model, c["X_new"], c["y_new"])
                B = c["sets"][which].astype(model.np_dtype)
                eta = rc.reference(name, dtype, which)["ref"]["eta"]
                for s in range(B.shape[0]):
                    pp.reset()
                    L = pp.update(B[s:s + 1]).table()[2]
                    nz = L > 0
                    if np.any(nz) and L[nz].min() < smallest[dtype][0]:
                        i = int(np.flatnonzero(nz)[np.argmin(L[nz])])
                        smallest[dtype] = (float(L[i]), float(abs(eta[s, i])), f"{name} {which}")
                    if np.any(~nz):
                        largest_zero[dtype] = max(largest_zero[dtype], float(np.max(np.exp(-np.abs(eta[s][~nz])))))
                pp.close()
        model.close()
        print(name, dtype, "  ".join(f"{k} {v:.3f}" for k, v in RATIOS[(name, dtype)].items()), flush=True)
    for d in rc.DTYPES:
        print(f"FIGURE smallest nonzero L {d}: {smallest[d][0]:.6e} at |t| = {smallest[d][1]} ({smallest[d][2]}); largest exp(-|t|) returned as 0: {largest_zero[d]:.6e}")
    for k in sorted({k for v in RATIOS.values() for k in v}):
        for d in rc.DTYPES:
            print(f"FIGURE largest ratio {k} {d}: {max(v.get(k, 0.0) for (n, dd), v in RATIOS.items() if dd == d):.3f}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--measure"]:
        sys.exit("usage: python tests/test_gpu_predict_regimes.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
