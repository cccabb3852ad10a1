"""The reference, the bounds and the cases of the saturated-logit tests of the draw-consuming kernels, checked without a GPU
(tests/pair_reference.py, tests/predict_regime_cases.py; the GPU side is tests/test_gpu_predict_regimes.py).

  - the per-pair reference (numpy.longdouble on the exact logit's head + residual) against mpmath at 50 digits, on a sample that
    covers every direction, every rung and both signs: relative 1e-15 on the longdouble values, which the float64 ones round
  - its table against predict_reference.reference_table (float64 mode) on the mixed set's draws with T <= 30, within the float64 bounds
  - the condition on the INPUTS: plain sequential NumPy arithmetic in the model's dtype (predict_reference._pairs, accumulated in
    longdouble) stays within 0.5 of every pair bound and every table bound, on every case, both dtypes and every set of draws.  The
    bounds are those of tests/pair_reference.py and are fitted to nothing
  - loo_reference.psis_table on the saturated log-likelihood matrices: no NaN and no warning; k-hat = inf wherever it is not finite,
    lppd = -inf exactly where every exp(l) underflows
  - every case reaches what it claims, the slicing of the host code included

`python tests/test_predict_regimes_cpu.py` prints the ratios of the third item per case.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_reference as er  # noqa: E402
import loo_reference as lref  # noqa: E402
import pair_reference as pref  # noqa: E402
import predict_reference as pr  # noqa: E402
import predict_regime_cases as rc  # noqa: E402

LD = np.longdouble
CASE_DTYPE = [(n, d) for n in rc.NAMES for d in rc.DTYPES]


def mpf_of(mp, v):
    """A longdouble as an mpf, exactly enough (the shortest decimal string that reads back as v: 21 digits)."""
    return mp.mpf(np.format_float_scientific(v, unique=True))


@pytest.mark.parametrize("name", rc.NAMES)
def test_pair_reference_matches_mpmath_at_50_digits(name):
    import mpmath  # (no importorskip: everything else rests on this test, and a skip would pass for a check)
    mp = mpmath.mp
    c = rc.case(name)
    dtype = rc.DTYPES[rc.NAMES.index(name) % 2]  # the rows as a float32 model holds them on the odd cases
    X = er.held(c["rows"], dtype)
    r = X.shape[0]
    rows = sorted({0, r // 2, r - 1})
    seen = set()
    with mp.workdps(50):
        xs = {i: [mp.mpf(float(v)) for v in X[i]] for i in rows}
        for which in rc.SETS:
            ref = rc.reference(name, dtype, which)["ref"]
            B = er.held(c["sets"][which], dtype)
            picks = range(24) if which == "mixed" else (0, rc.S_RUNG - 1)  # the first 24 draws of the mixed set are eval_cases.PAIRS
            for s in picks:
                b = [mp.mpf(float(v)) for v in B[s]]
                for i in rows:
                    eta = mp.fdot(xs[i], b)
                    sgn = 1 if c["labels"] is None else int(2 * c["labels"][i] - 1)
                    want = {"pi": 1 / (1 + mp.exp(-eta))}
                    if c["labels"] is not None:
                        t = sgn * eta
                        want["L"] = 1 / (1 + mp.exp(-t))
                        want["l"] = -mp.log1p(mp.exp(-t)) if t > -100 else t - mp.log1p(mp.exp(t))
                        seen.add((which, t > 0))
                    for k, w in want.items():
                        got = mpf_of(mp, ref["ld"][k][s, i])
                        assert abs(got - w) <= mp.mpf(1e-15) * abs(w), (name, dtype, which, s, i, k, got, w)
                        # the float64 value is the longdouble one rounded (below the normal range: to the subnormal grid)
                        assert abs(mp.mpf(float(ref[k][s, i])) - w) <= max(mp.mpf(2.0 ** -52) * abs(w), mp.mpf(5e-324)), (name, which, s, i, k)
                    assert abs(mp.mpf(float(ref["s"][s, i])) - mp.fsum(abs(x * bj) for x, bj in zip(xs[i], b))) <= mp.mpf(1e-15) * mp.mpf(float(ref["s"][s, i]))
    if c["labels"] is not None:
        assert {w for w, _ in seen} == set(rc.SETS)
        if r > 1:
            assert {pos for w, pos in seen if w == "mixed"} == {True, False}


@pytest.mark.parametrize("name", rc.NAMES)
def test_table_matches_the_float64_reference_table_in_the_tame_regime(name):
    c = rc.case(name)
    tame = [s for s, (_, T) in enumerate(c["pairs"]) if T <= 30]
    assert len(tame) >= 40
    B = c["sets"]["mixed"][tame]
    ref = pref.pairs(c["rows"], c["labels"], B, "float64")
    got = pr.reference_table(c["rows"], c["labels"], B)
    ratio = pref.ratio(got, pref.table(ref), pref.table_bounds(ref))
    assert ratio <= 1.0, (name, ratio)
    assert np.array_equal(np.isnan(got), np.isnan(pref.table(ref)))


def plain_arithmetic(name, dtype, which):
    """pi, L, l [S, r] by predict_reference._pairs in the model's dtype, and their table accumulated in longdouble."""
    c = rc.case(name)
    dt = np.dtype(dtype).type
    with np.errstate(under="ignore"):
        pi, L, l = pr._pairs(c["rows"].astype(dt), c["labels"], c["sets"][which].astype(dt), dt)
    vals = dict(pi=pi, L=L, l=l) if c["labels"] is not None else dict(pi=pi)
    tab = np.full((5, pi.shape[1]), np.nan)
    m, q, _ = pref._moments(pi.astype(LD))
    tab[0], tab[1] = m, q
    if c["labels"] is not None:
        tab[2] = L.astype(LD).sum(axis=0) / LD(L.shape[0])
        m, q, _ = pref._moments(l.astype(LD))
        tab[3], tab[4] = m, q
    return vals, tab


def plain_ratios(name, dtype):
    """Largest error / bound of plain arithmetic per quantity, over the sets of draws of a case."""
    out = {}
    for which in rc.SETS:
        R = rc.reference(name, dtype, which)
        vals, tab = plain_arithmetic(name, dtype, which)
        for k, v in vals.items():
            out[k] = max(out.get(k, 0.0), pref.ratio(v, R["ref"][k], R["tol"][k]))
        for row in range(5):
            out[f"row{row}"] = max(out.get(f"row{row}", 0.0), pref.ratio(tab[row], R["table"][row], R["ttol"][row]))
    return out


@pytest.mark.parametrize("name,dtype", CASE_DTYPE)
def test_plain_arithmetic_stays_within_half_of_every_bound(name, dtype):
    for k, v in plain_ratios(name, dtype).items():
        assert v <= 0.5, (name, dtype, k, v)


@pytest.mark.parametrize("name,dtype", CASE_DTYPE)
def test_psis_reference_is_clean_on_the_saturated_matrices(name, dtype):
    dt = np.dtype(dtype).type
    for which in rc.SETS:
        l = rc.reference(name, dtype, which, rows="model")["ref"]["l"].astype(dt)
        assert np.all(np.isfinite(l)) and np.all(l <= 0)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            t = lref.psis_table(l)
        assert not np.any(np.isnan(t[[0, 1, 3, 4]])), (name, dtype, which)
        assert np.all(np.isfinite(t[[0, 4]])) and np.all(np.isfinite(t[1]) | (t[1] == np.inf)) and np.all(np.isfinite(t[3]) | (t[3] == -np.inf))
        # n_eff = (sum w)^2 / sum w^2 as include/logreg_hip_loo.h defines it is 0 / 0 where every smoothed weight lies below 1e-162 and
        # the sum of squares underflows (a fitted tail whose scale is tiny under a cutoff of exp(-thousands); the header states the limit).
        # The rule, column by column: n_eff is NaN exactly where that sum is 0, finite everywhere else, and such a column has a fitted
        # k-hat far above 0.7.  (With the first draw of every design one column of one mixed set reaches it.)
        for i in range(t.shape[1]):
            _, lw = lref.psis_row(l[:, i], return_lw=True)
            with np.errstate(under="ignore"):
                underflowed = np.sum(np.exp(lw) ** 2) == 0.0
            assert np.isnan(t[2, i]) == underflowed and (underflowed or np.isfinite(t[2, i])), (name, dtype, which, i, t[2, i])
            assert not underflowed or (np.isfinite(t[1, i]) and t[1, i] > 0.7 and which == "mixed"), (name, dtype, which, i, t[1, i])
        with np.errstate(under="ignore"):
            dead = np.all(np.exp(l.astype(np.float64)) == 0, axis=0)
        assert np.array_equal(t[3] == -np.inf, dead), (name, dtype, which)
        assert np.all(t[4] <= lref.tail_length(l.shape[0]))
        if which != "mixed":  # nine draws: a tail of one, never fitted
            assert np.all(t[1] == np.inf) and np.all(t[4] <= 1)


@pytest.mark.parametrize("name", rc.NAMES)
def test_cases_reach_what_they_claim(name):
    c = rc.case(name)
    p, n, r = c["p"], c["n"], c["rows"].shape[0]
    assert c["X"].shape == (n, p) and c["sets"]["mixed"].shape == (rc.S_MIXED, p) and c["batchings"] in (("host", "device"), ("host_uneven", "device_uneven"))
    assert (c["X_new"] is None) == (c["kind"] == "own") and (c["labels"] is None) == (c["kind"] == "nolabels")
    if c["kind"] != "own":
        assert r == n - n // 3 != n and np.array_equal(c["X_new"], c["X"][::-1][:r])
    assert set(c["pairs"]) == set(rc.ec.PAIRS) and c["pairs"][:24] == rc.ec.PAIRS
    for dtype in rc.DTYPES:
        P, dg, chunked = rc.draws_in_flight(p, dtype)
        # the accumulator: more than one slice, each a pivot, whole groups and -- in some slice, where a group is more than a draw -- a remainder
        sl = rc.predict_slices(r, rc.S_MIXED)  # (one batch; the uneven batches are 1, 10, 73 = 37 + 36 and 50 draws)
        assert sl == [45, 45, 44] and all((k - 1) // dg >= 1 for k in sl) and (dg == 1 or any((k - 1) % dg for k in sl))
        assert rc.predict_slices(r, rc.S_RUNG) == [rc.S_RUNG]
        # the fill: more than one slice, the last one a partial tile; the nine draws of a rung are a partial tile of whole groups AND a
        # remainder whatever the group (9 = 2 x 4 + 1 = 4 x 2 + 1 = 8 + 1)
        fs, ts = rc.fill_slices(n, rc.S_MIXED, dtype)
        assert fs == [64, 64, 6] and fs[-1] < ts
        assert rc.fill_slices(n, rc.S_RUNG, dtype)[0] == [rc.S_RUNG] and ts > rc.S_RUNG >= dg and (dg == 1 or rc.S_RUNG % dg)
        mixed = rc.reference(name, dtype, "mixed")["ref"]
        for s, (which, T) in enumerate(c["pairs"]):
            assert np.max(np.abs(mixed["eta"][s])) == pytest.approx(T, rel=1e-4 if dtype == "float32" else 1e-12)
        for T in rc.RUNGS:
            R = rc.reference(name, dtype, f"T{T}")
            eta = R["ref"]["eta"]
            top = np.max(np.abs(eta), axis=1)
            assert top[-1] == pytest.approx(T, rel=1e-4) and top[0] == pytest.approx(0.9 * T, rel=1e-4) and np.all(np.diff(top) > 0)
            if c["labels"] is not None:  # every row on the wrong side in every draw
                t = eta * R["ref"]["sign"][None, :]
                assert np.all(t <= 0) and np.all(R["ref"]["L"] <= 0.5)
                i = int(np.argmin(t[-1]))
                assert R["table"][2, i] <= np.exp(-0.899 * T), (name, dtype, T)  # the mean of L is tiny (0 in float64 at T = 5000)
    # the clamps and the edges of the number formats are straddled by the mixed set and hit by the rungs
    eta32 = np.abs(rc.reference(name, "float32", "mixed")["ref"]["eta"])
    eta64 = np.abs(rc.reference(name, "float64", "mixed")["ref"]["eta"])
    for lo, hi in ((87.4, 103.9), (103.98, 130.0), (600.0, 708.0), (750.0, 5001.0)):
        assert np.any((eta32 > lo) & (eta32 <= hi)) or r == 1 and lo in (87.4, 600.0), (name, lo)
        assert np.any((eta64 > lo) & (eta64 <= hi)) or r == 1 and lo in (87.4, 600.0), (name, lo)
    sub = np.abs(rc.reference(name, "float32", "T90")["ref"]["eta"])
    assert np.any((sub > 87.4) & (sub < 103.9))  # float32 L = exp(-|t|) between 2^-149 and 2^-126


if __name__ == "__main__":
    for nm, dty in CASE_DTYPE:
        print(nm, dty, "  ".join(f"{k} {v:.3f}" for k, v in plain_ratios(nm, dty).items()), flush=True)
