"""Bridge sampling on the device (include/logreg_hip_bridge.h, logreg_amd/bridge.py) against tests/bridge_reference.py: the terms at
every width boundary and across a row slice, the proposal draws, the iteration, bit exactness of batchings, reruns and builds, and the
log marginal likelihood end to end against quadrature and against the importance-sampling fixture."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import bridge_reference as br

pytestmark = pytest.mark.gpu

WIDTHS, ROWS, CALLS = br.WIDTHS, br.ROWS, br.CALLS
DT = {"float32": np.float32, "float64": np.float64}


def note(line):  # the figures behind every assertion, for the profile file (run with -s)
    print(line)


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


def feed(acc, B, cuts, kind="host"):
    from logreg_amd import DeviceArray
    i = 0
    for c in cuts:
        blk = B[i:i + c]
        if kind == "device":
            d = DeviceArray.from_host(acc.device, np.ascontiguousarray(blk, dtype=acc.dtype))
            acc.update(d)
            acc.terms()  # (synchronises: the block may go)
            d.free()
        else:
            acc.update(blk)
        i += c
    assert i == B.shape[0]
    return acc


# ---- 1. terms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("p", WIDTHS)
def test_terms_against_the_reference(la, p, dtype):
    """l1 of sum(CALLS) draws fed in calls of 1, 33 and 1025, and l2 of the accumulator's own proposal draws, at every n of ROWS.
    float64: |device - reference| <= bridge_reference.term_bound64, derived from the inputs (n row terms and p^2 Gaussian terms, 4 ulp of
    each magnitude).  float32: <= F32_UNITS[n] float32 ulps of the rows' magnitudes, the bound measured on the CPU on these cases (test_bridge_cpu.py)."""
    dt = DT[dtype]
    for n in ROWS:
        c = br.rounded(br.gpu_term_case(p, n), dt)
        model = la.LogReg(c["X"], c["y"], c["pscale"], dtype=dtype)
        acc = la.Bridge(model, c["mu"], c["cov"], max_draws=sum(CALLS), n_proposal=130, seed=5)
        feed(acc, c["B"], CALLS)
        l1, l2 = acc.terms()
        prop = acc.proposal_draws().astype(np.float64)
        for got, B, what in ((l1, c["B"], "l1"), (l2, prop, "l2")):
            ref = br.terms(c["X"], c["y"], c["pscale"], B, c["mu"], c["cov"], "float64")
            bound = br.term_bound64(c["X"], c["pscale"], B, c["mu"], c["cov"]) if dtype == "float64" else br.F32_UNITS[n] * br.term_unit32(c["X"], B)
            worst = float(np.max(np.abs(got - ref) / bound))
            note(f"[bridge] terms {what} p={p} n={n} {dtype}: worst |dev - ref| / bound = {worst:.3e} (max |dev - ref| {np.max(np.abs(got - ref)):.3e})")
            assert np.all(np.isfinite(got)) and worst <= 1.0, (p, n, dtype, what, worst)
        acc.close()
        model.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_saturated_logits_and_non_finite_draws(la, dtype):
    """Logits up to +-5000 stay finite and agree with the reference; a NaN and an inf coordinate give non-finite terms exactly where the
    reference has them, the count matches and logml is NaN."""
    dt = DT[dtype]
    c = br.rounded(br.saturated_case(), dt)
    mu, cov = c["mu"], c["cov"]
    model = la.LogReg(c["X"], c["y"], c["pscale"], dtype=dtype)
    acc = la.Bridge(model, mu, cov, max_draws=64, n_proposal=50, seed=1)
    l1, _ = acc.update(c["B"]).terms()
    ref = br.terms(c["X"], c["y"], c["pscale"], c["B"], mu, cov, "float64")
    assert np.all(np.isfinite(l1)) and np.max(np.abs(c["X"] @ c["B"].T)) > 4000
    tol = br.term_bound64(c["X"], c["pscale"], c["B"], mu, cov) if dtype == "float64" else br.F32_UNITS["saturated"] * br.term_unit32(c["X"], c["B"])
    assert np.all(np.abs(l1 - ref) <= tol), float(np.max(np.abs(l1 - ref) / tol))
    ok = acc.result()
    assert np.isfinite(ok["logml"]) and ok["n_nonfinite"] == 0
    bad = c["B"][:6].copy()
    bad[1, 2], bad[4, 0] = np.nan, np.inf
    acc.update(bad)
    l1, l2 = acc.terms()
    with np.errstate(all="ignore"):
        ref = br.terms(c["X"], c["y"], c["pscale"], np.concatenate([c["B"], bad]), mu, cov, "float64")
    assert np.array_equal(np.isfinite(l1), np.isfinite(ref)) and np.sum(~np.isfinite(l1)) == 2
    res = acc.result()
    assert np.isnan(res["logml"]) and np.isnan(res["se"]) and res["n_nonfinite"] == 2 == br.solve(l1, l2)["n_nonfinite"]
    assert res["l1_min"] == np.min(l1[np.isfinite(l1)]) and res["l1_max"] == np.max(l1[np.isfinite(l1)])
    acc.close()
    model.close()


# ---- 2. proposal draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_proposal_draws_against_the_philox_restatement(la, dtype):
    """theta~ = mu + L z: the device's normals are within 4e-6 (float32: hardware transcendentals; the tolerance of
    test_gpu_parity.py::test_device_normals_against_the_oracle) / 1e-12 (float64) of the float64 Box-Muller on the same Philox words, so
    coordinate i is within that x sum_k |L_ik|, plus the rounding of theta to the model's dtype."""
    dt = DT[dtype]
    for p in (3, 17, 128):
        c = br.term_case(p, 8, seed=p)
        model = la.LogReg(c["X"], c["y"], c["pscale"], dtype=dtype)
        a2 = la.Bridge(model, c["mu"], c["cov"], max_draws=4, n_proposal=2000, seed=77)
        a1 = la.Bridge(model, c["mu"], c["cov"], max_draws=4, n_proposal=1000, seed=77)
        a3 = la.Bridge(model, c["mu"], c["cov"], max_draws=4, n_proposal=1000, seed=78)
        d2, d1, d3 = a2.proposal_draws(), a1.proposal_draws(), a3.proposal_draws()
        assert d2.dtype == dt and d2[:1000].tobytes() == d1.tobytes()  # draw j depends on (seed, j) alone
        assert a2.terms()[1][:1000].tobytes() == a1.terms()[1].tobytes()
        assert not np.any(np.all(d3 == d1, axis=1))  # another seed, other draws
        ref = br.proposal_draws(77, 2000, c["mu"], c["cov"])
        L, _ = br.factor(c["cov"])
        ztol = 4e-6 if dtype == "float32" else 1e-12
        tol = ztol * np.sum(np.abs(L), axis=1)[None, :] + (2.0 ** -23 if dtype == "float32" else 2.0 ** -51) * np.abs(ref)
        worst = float(np.max(np.abs(d2.astype(np.float64) - ref) / tol))
        note(f"[bridge] proposal draws p={p} {dtype}: worst deviation / tolerance {worst:.3e}")
        assert worst <= 1.0, (p, dtype, worst)
        z = np.linalg.solve(L, (d2.astype(np.float64) - c["mu"]).T).T  # and they ARE standard normal: moments of 2000 p values
        assert abs(np.mean(z)) < 5 / np.sqrt(z.size) and abs(np.var(z) - 1) < 5 * np.sqrt(2 / z.size)
        for a in (a1, a2, a3):
            a.close()
        model.close()


# ---- 3. iteration ------------------------------------------------------------------------------------------------------------------------------
def _small(la, dtype="float64", S=6000, N2=5000, seed=0):
    X, y, ps = br.small_model(0)
    b, C = br.newton_mode(X, y, ps)
    rng = np.random.default_rng(seed)
    B = b + rng.standard_normal((S, 2)) @ np.linalg.cholesky(C).T  # posterior-like draws (the Laplace approximation's)
    model = la.LogReg(X, y, ps, dtype=dtype)
    acc = la.Bridge(model, b, 1.2 * C, max_draws=S, n_proposal=N2, seed=seed)
    return model, acc, B


@pytest.mark.parametrize("tau", [1e-10, 1e-6])
def test_iteration_against_the_reference_on_the_devices_own_terms(la, tau):
    model, acc, B = _small(la)
    l1, l2 = acc.update(B).terms()
    for n_eff in (None, 1500.0):
        ref = br.solve(l1, l2, n_eff=n_eff, tol=tau)
        res = acc.result(n_eff=n_eff, tol=tau)
        d = np.abs(np.diff(ref["trace"]))
        ratios = d[1:] / d[:-1]
        note(f"[bridge] iteration tau={tau:g} n_eff={n_eff}: reference {ref['iterations']} iterations, contraction ratios {np.round(ratios, 4)}; "
             f"device {res['iterations']} iterations, |dlogml| {abs(res['logml'] - ref['logml']):.3e}, se rel {abs(res['se'] / ref['se'] - 1):.3e}")
        assert len(ratios) >= 1 and np.all(ratios[d[:-1] > 1e-12] < 0.5)  # the case contracts: the 4 tau bound below holds
        assert ref["converged"] and res["converged"]
        # each side's stopping error is at most tau max(1, |logml|) (ratio < 1/2) and the stops may differ by one step
        assert abs(res["logml"] - ref["logml"]) <= 4 * tau * max(1.0, abs(ref["logml"]))
        assert abs(res["iterations"] - ref["iterations"]) <= 1
        assert abs(res["se"] / ref["se"] - 1) <= 1e-9
        assert res["n_eff"] == (n_eff or l1.size) and res["n_draws"] == l1.size and res["n_proposal"] == l2.size
        solo = la.bridge_from_terms(l1, l2, n_eff=n_eff, tol=tau)
        assert solo["table"].tobytes() == res["table"].tobytes()  # lr_bridge_solve: the same bytes
    few = acc.result(maxit=0)  # the plain importance-sampling start
    assert few["iterations"] == 0 and not few["converged"] and abs(few["logml"] - br.solve(l1, l2, maxit=0)["logml"]) < 1e-12
    c = la.bridge_from_terms(np.full(300, -7.25), np.full(5000, -7.25))
    assert c["logml"] == -7.25 and c["iterations"] == 1 and c["converged"]  # equal terms: exactly c after one iteration
    acc.close()
    model.close()


# ---- 4. bytes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_batchings_reruns_sources_and_both_builds_give_identical_bytes(la, dtype):
    from logreg_amd import _lib
    import altlib
    c = br.rounded(br.term_case(17, 601, seed=9, S=1500), DT[dtype])

    def run(cuts, kind="host", again=False):
        model = la.LogReg(c["X"], c["y"], c["pscale"], dtype=dtype)
        acc = la.Bridge(model, c["mu"], c["cov"], max_draws=1500, n_proposal=700, seed=3)
        feed(acc, c["B"], cuts, kind)
        out = [acc.terms(), acc.table(n_eff=400.0)]
        if again:  # reset, then refill: the same bytes, the proposal terms kept
            acc.reset()
            assert acc.n_draws == 0 and np.isnan(acc.result()["logml"])
            feed(acc, c["B"], cuts, kind)
            out += [acc.terms(), acc.table(n_eff=400.0)]
        acc.close()
        model.close()
        return out

    def same(a, b):
        return a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1].tobytes() and a[1].tobytes() == b[1].tobytes()
    one = run([1500], again=True)
    assert same(one[:2], one[2:])
    assert same(one, run([1, 1024, 475])) and same(one, run([1500])) and same(one, run([700, 800], kind="device"))
    L = altlib.install()
    try:
        _lib.bind_bridge(L)
        assert _lib.load() is L
        alt = run([1500])
    finally:
        altlib.uninstall()
        _lib.bind_bridge(_lib.load())
    assert same(one, alt)


def test_host_draws_one_longer_than_a_staging_piece_give_the_bytes_of_two_updates(la):
    """Draws are staged in pieces of max(1024, 256 MB / (P esize)): P = 128 float64 -> 262144 draws.  One update of a draw more is the
    launch sequence of two updates cut there.  (A change of the 256 MB needs another shape here.)"""
    p, piece = 128, 262144
    rng = np.random.default_rng(14)
    X = rng.standard_normal((8, p))
    y = (rng.random(8) < 0.5).astype(np.float64)
    B = 0.05 * rng.standard_normal((piece + 1, p))
    model = la.LogReg(X, y, np.full(p, 2.0), dtype="float64")
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        acc = la.Bridge(model, np.zeros(p), 0.0025 * np.eye(p), max_draws=piece + 1, n_proposal=64, seed=1)
        feed(acc, B, cuts)
        out.append((acc.terms()[0], acc.table()))
        acc.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    ref = br.terms(X, y, np.full(p, 2.0), B[-3:], np.zeros(p), 0.0025 * np.eye(p))
    assert np.all(np.abs(out[0][0][-3:] - ref) <= br.term_bound64(X, np.full(p, 2.0), B[-3:], np.zeros(p), 0.0025 * np.eye(p)))
    model.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------
def _two_halves(la, model, kern, start, iters, seed, p, dtype, center, sd):
    """Covariance on the first half gives the proposal; Bridge and Autocorr run on the second half -> (result, Bridge)"""
    chains = start.shape[0]
    center, scale = la.covariance_scaling(center, sd)
    cov = la.Covariance(chains, p, dtype=dtype, center=center, scale=scale)
    first = la.mcmc(start, kern, thin=1, iters=iters, verb=False, seed=seed, summary_only=True, covariance=cov)
    mean, S = la.bridge_proposal(first["covariance"])
    acc = la.Bridge(model, mean, S, max_draws=iters * chains, seed=seed)
    ac = la.Autocorr(chains, p, dtype=dtype)
    second = la.mcmc(first["state"], kern, thin=1, iters=iters, verb=False, seed=seed + 1, summary_only=True, bridge=acc, autocorr=ac)
    assert second["bridge"]["n_draws"] == iters * chains and second["bridge"]["converged"]
    n_eff = float(np.min(second["autocorr"]["ess"]))
    cov.free()
    ac.free()
    return acc.result(n_eff=n_eff), acc


def test_small_model_against_quadrature(la):
    """The 30 x 2 model: 64 chains of pgKernel, 400 kept sweeps, the proposal from the first 200, the terms from the last 200, n_eff from
    Autocorr.  |logml - quadrature| <= 5 se."""
    X, y, ps = br.small_model(0)
    truth = br.quadrature_logml(X, y, ps)
    model = la.LogReg(X, y, ps, dtype="float64")
    b, C = br.newton_mode(X, y, ps)
    res, acc = _two_halves(la, model, la.pgKernel(model.lpost), np.tile(b, (64, 1)), 200, 11, 2, "float64", b, np.sqrt(np.diag(C)))
    z = (res["logml"] - truth) / res["se"]
    note(f"[bridge] 30 x 2 model: quadrature {truth:.6f}, bridge {res['logml']:.6f} +- {res['se']:.2e} (n_eff {res['n_eff']:.0f} of {res['n_draws']}, "
         f"{res['iterations']} iterations), z = {z:+.3f}")
    assert res["converged"] and res["se"] < 0.02 and abs(z) <= 5.0
    acc.close()
    model.close()


def test_pima_against_the_importance_sampling_fixture_and_a_dropped_column(la, pima, pscale):
    """Pima, float64, NUTS after nuts_warmup: logml within 5 combined standard errors of tests/golden/bridge_pima.json (a 6 x 10^5-draw
    float64 importance sampler), for the full design and for the design with one column dropped; bridge_compare has the fixture's sign and
    size."""
    with open(os.path.join(GOLDEN, "bridge_pima.json")) as f:
        fx = json.load(f)
    X, y = pima
    keep = [j for j in range(X.shape[1]) if j != fx["drop"]]
    got = {}
    for name, cols in (("full", list(range(X.shape[1]))), ("dropped", keep)):
        model = la.LogReg(X[:, cols], y, pscale[cols], dtype="float64")
        warm = la.nuts_warmup(model.lpost, model.glp, np.zeros((64, len(cols))), num_warmup=300, seed=21)
        beta, info = la.find_map(model)
        res, acc = _two_halves(la, model, warm.kernel, warm.state, 150, 31, len(cols), "float64", beta, info["sd"])
        d, s = res["logml"] - fx[name]["logml"], np.sqrt(res["se"] ** 2 + fx[name]["se"] ** 2)
        note(f"[bridge] pima {name}: fixture {fx[name]['logml']:.5f} +- {fx[name]['se']:.1e}, bridge {res['logml']:.5f} +- {res['se']:.1e} "
             f"(n_eff {res['n_eff']:.0f} of {res['n_draws']}), z = {d / s:+.3f}")
        assert res["converged"] and abs(d) <= 5 * s, (name, d, s)
        got[name] = res
        acc.close()
        model.close()
    cmp = la.bridge_compare(got["full"], got["dropped"])
    want = fx["log_bf_full_vs_dropped"]
    s = np.sqrt(cmp["se"] ** 2 + fx["full"]["se"] ** 2 + fx["dropped"]["se"] ** 2)
    note(f"[bridge] pima log Bayes factor full vs dropped: fixture {want:+.4f}, bridge {cmp['log_bf']:+.4f} +- {cmp['se']:.1e}")
    assert np.sign(cmp["log_bf"]) == np.sign(want) and abs(cmp["log_bf"] - want) <= 5 * s
