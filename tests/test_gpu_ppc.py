"""Posterior predictive checks on the device (include/logreg_hip_ppc.h, logreg_amd/ppc.py) against tests/ppc_reference.py: the replicate
of every decided pair, the counts against the device's own bits, the deviances within bounds derived from the inputs, the accumulated
tables against a host recount, byte identity of the integer tables across cuts, pieces, sub-batches, pointer kinds, reruns and builds,
saturated and non-finite input, mcmc(check=), and the statistics end to end."""
import numpy as np
import pytest

import ppc_cases as pc
import ppc_reference as ppr

pytestmark = pytest.mark.gpu

INT_TABLES = ("hist", "row_ones", "counts")
CASE_IDS = ["r%d_p%d_S%d" % c for c in pc.CASES]


def note(line):  # the figures behind every assertion (run with -s)
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
            d = DeviceArray.from_host(acc.model.device, np.ascontiguousarray(blk, dtype=acc.model.np_dtype))
            acc.update(d)
            acc.tables()  # (synchronises: the block may go)
            d.free()
        else:
            acc.update(blk)
        i += c
    assert i == B.shape[0]
    return acc


def same_ints(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in INT_TABLES) and a["n_draws"] == b["n_draws"]


def laplace_draws(X, y, sd, S, seed):
    import bridge_reference as br
    b, C = br.newton_mode(X, y, sd)
    return b + np.random.default_rng(seed).standard_normal((S, X.shape[1])) @ np.linalg.cholesky(C).T


# ---- 1. terms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("case", pc.CASES, ids=CASE_IDS)
def test_terms_against_the_reference(la, case, dtype):
    """Draws taken as s = FIRST .. (both end quads partial), seven groups with the last empty: every decided pair's bit is the
    reference's; counts_out is the popcount of the device's own bits per group; D_obs and D_rep (the latter for the device's own bits)
    within the summed pair bounds of l plus the float64 summation term."""
    r, p, S = case
    ref = pc.reference(r, p, S, dtype)
    G = 7 if r > 1 else 1
    groups = pc.groups_for(r, G)
    model = la.LogReg(ref["X"], ref["y"], np.ones(p), dtype=dtype)
    acc = la.PredictiveCheck(model, groups=groups, seed=pc.SEED, n_groups=G)
    counts, dev, bits = acc.terms(ref["B"], first_index=pc.FIRST)
    rep = ppr.unpack(bits, r)
    ok = ~ref["undecided"]
    wrong = int(np.sum(rep[ok] != ref["rep"][ok]))
    note(f"[ppc] terms {case} {dtype}: {int((~ok).sum())} of {ok.size} pairs undecided, {wrong} decided pairs differ")
    assert wrong == 0
    assert np.array_equal(counts, ppr.counts_of(rep, groups, G))
    pad = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, r:]
    assert not pad.any()  # the bits past r
    for k, lab in ((0, ref["y"] > 0.5), (1, rep)):
        D, bound = ppr.deviance(ref["pv"], lab)
        q = float(np.max(np.abs(dev[:, k] - D) / bound))
        note(f"[ppc]   D_{'obs' if k == 0 else 'rep'}: worst |device - reference| / bound = {q:.3f}")
        assert q <= 1.0
    assert acc.n_draws == 0 and acc.result()["n_draws"] == 0  # nothing was accumulated
    acc.close()
    model.close()


def test_terms_without_labels_and_on_rows_of_its_own(la):
    """X_new without y_new: D_obs is NaN, D_rep and the bits are those of the labelled accumulator on the same rows."""
    r, p, S = pc.CASES[2]
    ref = pc.reference(r, p, S, "float32")
    model = la.LogReg(ref["X"][:40], ref["y"][:40], np.ones(p), dtype="float32")
    lab, unl = la.PredictiveCheck(model, ref["X"], ref["y"], seed=pc.SEED), la.PredictiveCheck(model, ref["X"], seed=pc.SEED)
    c1, d1, b1 = lab.terms(ref["B"], first_index=pc.FIRST)
    c0, d0, b0 = unl.terms(ref["B"], first_index=pc.FIRST)
    assert np.array_equal(b0, b1) and np.array_equal(c0, c1) and np.all(np.isnan(d0[:, 0])) and np.array_equal(d0[:, 1], d1[:, 1])
    ok = ~ref["undecided"]
    assert np.array_equal(ppr.unpack(b1, r)[ok], ref["rep"][ok])
    res = unl.update(ref["B"]).result()
    assert res["t_obs"].tolist() == [-1] and np.isnan(res["dev_p"]) and np.isnan(res["dev_obs_mean"]) and np.isfinite(res["dev_rep_mean"])
    for a in (lab, unl):
        a.close()
    model.close()


# ---- 2. accumulation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("case", pc.CASES, ids=CASE_IDS)
def test_accumulation_equals_a_host_recount_of_terms(la, case, dtype):
    """hist, row_ones and dev_ge of draws fed in three calls equal a host recount of the outputs of terms, exactly; the moment rows are
    within the float64 accumulation term of pair_reference.table_bounds."""
    r, p, S = case
    ref = pc.reference(r, p, S, dtype)
    G = 7 if r > 1 else 1
    groups = pc.groups_for(r, G)
    model = la.LogReg(ref["X"], ref["y"], np.ones(p), dtype=dtype)
    acc = la.PredictiveCheck(model, groups=groups, seed=pc.SEED, n_groups=G)
    counts, dev, bits = acc.terms(ref["B"])
    feed(acc, ref["B"], [3, 6, S - 9])
    t = acc.tables()
    want = ppr.accumulate(counts, dev, ppr.unpack(bits, r), t["n_g"])
    assert same_ints(t, want)
    q = float(np.max(np.abs(t["moments"] - want["moments"]) / ppr.moment_bounds(dev)))
    note(f"[ppc] moments {case} {dtype}: worst |device - two-pass| / bound = {q:.3f}")
    assert q <= 1.0
    res = acc.result()
    assert [int(h.sum()) for h in res["hist"]] == [S] * G and res["n_g"].tolist() == np.bincount(groups if groups is not None else np.zeros(r, int), minlength=G).tolist()
    assert res["t_obs"].tolist() == [int(ref["y"][(groups if groups is not None else np.zeros(r, int)) == g].sum()) for g in range(G)]
    acc.close()
    model.close()


# ---- 3. cuts, pieces, pointers, reruns, builds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_cuts_pointers_reruns_and_both_builds_give_identical_integer_tables(la, dtype):
    """1025 draws in one call against calls of 1, 5, 33 and 986 (call starts at s mod 4 = 1, 2, 3), device pointers, a rerun after
    reset (the moments too: the same sequence of calls), and the second build."""
    from logreg_amd import _lib
    import altlib
    r, p, S = 257, 17, 1025
    X, y, B = pc.data(r, p, S)
    groups = pc.groups_for(r, 2)

    def run(cuts, kind="host", again=False):
        model = la.LogReg(X, y, np.ones(p), dtype=dtype)
        acc = la.PredictiveCheck(model, groups=groups, seed=3, n_groups=2)
        out = [feed(acc, B, cuts, kind).tables()]
        if again:
            acc.reset()
            assert acc.result()["n_draws"] == 0 and int(acc.tables()["hist"].sum()) == 0
            out.append(feed(acc, B, cuts, kind).tables())
        acc.close()
        model.close()
        return out
    one, again = run([1025], again=True)
    assert same_ints(one, again) and one["moments"].tobytes() == again["moments"].tobytes()
    for cuts, kind in (([1, 5, 33, 986], "host"), ([1, 5, 33, 986], "device"), ([1025], "device"), ([2, 1, 1022], "host")):
        other = run(cuts, kind)[0]
        assert same_ints(one, other), (cuts, kind)
        assert np.allclose(one["moments"], other["moments"], rtol=1e-12, atol=0)
    assert one["moments"].tobytes() == run([1025], "device")[0]["moments"].tobytes()  # the pointer kind alone changes nothing
    L = altlib.install()
    try:
        _lib.bind_ppc(L)
        assert _lib.load() is L
        alt = run([1025])[0]
    finally:
        altlib.uninstall()
        _lib.bind_ppc(_lib.load())
    assert same_ints(one, alt)


def test_a_sub_batch_boundary_moves_no_integer(la):
    """100 003 rows: 391 tiles, 20 bytes per (tile, draw) of 64 MB -> sub-batches of 8580 draws.  8587 draws in one call and cut after
    3 draws run as different launch sequences; the integer tables agree, and with a recount of terms' counts."""
    r, p, S = 100003, 3, 8587
    rng = np.random.default_rng(5)
    X = np.concatenate([np.ones((r, 1)), rng.standard_normal((r, p - 1))], axis=1)
    y = (rng.random(r) < 0.4).astype(np.float64)
    B = np.array([-0.4, 0.5, -0.3]) + 0.05 * rng.standard_normal((S, p))
    model = la.LogReg(X, y, np.ones(p), dtype="float32")
    out = []
    for cuts in ([S], [3, S - 3]):
        acc = la.PredictiveCheck(model, seed=8)
        out.append(feed(acc, B, cuts).tables())
        if len(out) == 1:
            counts, dev, _ = acc.terms(B, bits=False)
        acc.close()
    assert same_ints(out[0], out[1]) and np.allclose(out[0]["moments"], out[1]["moments"], rtol=1e-12, atol=0)
    assert np.array_equal(np.bincount(counts[:, 0], minlength=r + 1).astype(np.uint64), out[0]["hist"])
    assert int(out[0]["counts"][0]) == int(np.sum(dev[:, 1] >= dev[:, 0])) and int(out[0]["row_ones"].sum()) == int(counts.sum())
    model.close()


def test_host_draws_one_longer_than_a_staging_piece_give_the_tables_of_two_updates(la):
    """Draws are staged in pieces of max(1024, 256 MB / (P esize)): P = 128 float64 -> 262144 draws.  One update of a draw more is the
    launch sequence of two updates cut there: every table byte for byte, the moments too."""
    p, piece = 128, 262144
    rng = np.random.default_rng(14)
    X = rng.standard_normal((8, p))
    y = (rng.random(8) < 0.5).astype(np.float64)
    B = 0.05 * rng.standard_normal((piece + 1, p))
    model = la.LogReg(X, y, np.full(p, 2.0), dtype="float64")
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        acc = la.PredictiveCheck(model, seed=1)
        out.append(feed(acc, B, cuts).tables())
        acc.close()
    assert same_ints(out[0], out[1]) and out[0]["moments"].tobytes() == out[1]["moments"].tobytes() and int(out[0]["hist"].sum()) == piece + 1
    model.close()


# ---- 4. groups ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", pc.GROUPS)
def test_groups_interleaved_across_tiles_with_one_empty(la, G):
    r, p, S = pc.CASES[4]
    ref = pc.reference(r, p, S, "float32")
    groups = pc.groups_for(r, G)
    model = la.LogReg(ref["X"], ref["y"], np.ones(p), dtype="float32")
    acc = la.PredictiveCheck(model, groups=groups, seed=pc.SEED, n_groups=G)
    counts, dev, bits = acc.terms(ref["B"], first_index=pc.FIRST)
    rep = ppr.unpack(bits, r)
    assert counts.shape == (S, G) and np.array_equal(counts, ppr.counts_of(rep, groups, G))
    ok = ~ref["undecided"]
    assert np.array_equal(rep[ok], ref["rep"][ok])  # the groups move no replicate
    res = acc.update(ref["B"]).result()
    assert res["n_g"].sum() == r and (G == 1 or res["n_g"][-1] == 0) and [int(h.sum()) for h in res["hist"]] == [S] * G
    if G > 1:
        assert res["hist"][-1].tolist() == [S] and res["p_two"][-1] == 1.0  # the empty group: T = 0 = T_obs in every draw
    acc.close()
    model.close()


# ---- 5. saturated and non-finite input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_saturated_logits_give_deterministic_replicates_and_finite_deviances(la, dtype):
    """Logits of +-5000: pi is 0 or 1 (or below every uniform), the replicate is [eta > 0] whatever the uniform, D_rep = 0 and
    D_obs = 2 x 5000 per mislabelled row, both finite."""
    r, S = 63, 70
    sgn = np.where(np.arange(r) % 3 == 0, -1.0, 1.0)
    X = np.stack([sgn, np.zeros(r)], axis=1)
    y = (np.arange(r) % 2).astype(np.float64)
    B = np.tile([[5000.0, 0.25]], (S, 1))
    model = la.LogReg(X, y, np.ones(2), dtype=dtype)
    acc = la.PredictiveCheck(model, seed=2)
    counts, dev, bits = acc.terms(B)
    rep = ppr.unpack(bits, r)
    assert np.array_equal(rep, np.tile(sgn > 0, (S, 1))) and np.all(counts[:, 0] == int((sgn > 0).sum()))
    wrong = int(np.sum((sgn > 0) != (y > 0.5)))
    assert np.all(np.isfinite(dev)) and np.all(np.abs(dev[:, 1]) < 1e-300) and np.all(dev[:, 0] == 2 * 5000.0 * wrong)  # (exp(-750) may be a subnormal)
    res = acc.update(B).result()
    assert res["dev_p"] == 0.0 and res["n_nonfinite"] == 0 and res["sd"][0] == 0.0
    acc.close()
    model.close()


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_a_nonfinite_draw_is_counted_consumes_its_index_and_moves_nothing_else(la, dtype):
    r, p, S = pc.CASES[2]
    ref = pc.reference(r, p, S, dtype)
    model = la.LogReg(ref["X"], ref["y"], np.ones(p), dtype=dtype)
    acc = la.PredictiveCheck(model, seed=pc.SEED)
    clean = acc.terms(ref["B"])
    bad = ref["B"].copy()
    bad[30, 2], bad[41, 0] = np.nan, np.inf
    counts, dev, bits = acc.terms(bad)
    keep = np.ones(S, dtype=bool)
    keep[[30, 41]] = False
    assert np.array_equal(counts[keep], clean[0][keep]) and np.array_equal(dev[keep], clean[1][keep]) and np.array_equal(bits[keep], clean[2][keep])
    assert not counts[~keep].any() and not bits[~keep].any() and np.all(np.isnan(dev[~keep]))
    t = feed(acc, bad, [29, 2, S - 31]).tables()
    want = ppr.accumulate(counts, dev, ppr.unpack(bits, r), t["n_g"], finite=keep)
    assert same_ints(t, want) and t["counts"][1] == 2 and t["n_draws"] == S
    assert np.max(np.abs(t["moments"] - want["moments"]) / ppr.moment_bounds(dev[keep])) <= 1.0
    res = acc.result()
    assert res["n"] == S - 2 and res["n_nonfinite"] == 2 and np.isfinite(res["dev_rep_mean"]) and int(res["hist"][0].sum()) == S - 2
    acc.close()
    model.close()


# ---- 6. mcmc ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("summary_only", [False, True])
def test_mcmc_check_equals_feeding_the_returned_samples_by_hand(la, pima, pscale, summary_only):
    X, y = pima
    model = la.LogReg(X, y, pscale, dtype="float32")
    groups = (np.arange(X.shape[0]) % 3).astype(np.int32)
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-2, l=8, dmm=1.0 / pscale ** 2)
    init = np.zeros((64, 8))
    acc = la.PredictiveCheck(model, groups=groups, seed=21)
    out = la.mcmc(init, kern, thin=2, iters=30, verb=False, seed=4, chunk=7)
    if summary_only:
        got = la.mcmc(init, kern, thin=2, iters=30, verb=False, seed=4, chunk=7, summary_only=True, check=acc)["check"]
    else:
        out2, info = la.mcmc(init, kern, thin=2, iters=30, verb=False, seed=4, chunk=7, return_info=True, check=acc)
        assert out2.tobytes() == out.tobytes()  # the chains are those of the same call without it
        got = info["check"]
    by_hand = la.PredictiveCheck(model, groups=groups, seed=21).update(out).tables()
    assert got["n_draws"] == 30 * 64 and same_ints(got["tables"], by_hand)
    for a in (acc,):
        a.close()
    model.close()


# ---- 7. statistics ---------------------------------------------------------------------------------------------------------------------------------
def test_replicated_count_on_pima_agrees_with_the_predictive_mean(la, pima, pscale):
    """|mean T_rep - sum_i mean pi_i| <= 6 sqrt(n / (4 S)): T_rep(s) has variance <= n / 4 given the draw, so its mean over S draws has
    a standard deviation of at most sqrt(n / (4 S)) around the mean of sum_i pi_i(s), which PosteriorPredictive gives on the same draws."""
    X, y = pima
    n, S = X.shape[0], 4000
    draws = laplace_draws(X, y, pscale, S, 3)
    model = la.LogReg(X, y, pscale, dtype="float32")
    acc, pp = la.PredictiveCheck(model, seed=77), la.PosteriorPredictive(model)
    res = acc.update(draws).result()
    mean_pi = pp.update(draws).proba()[0]
    gap, bound = abs(res["mean"][0] - mean_pi.sum()), 6 * np.sqrt(n / (4 * S))
    note(f"[ppc] Pima: mean T_rep {res['mean'][0]:.3f}, sum of mean pi {mean_pi.sum():.3f}, observed {res['t_obs'][0]}, gap {gap:.3f} <= {bound:.3f}")
    assert gap <= bound
    assert np.max(np.abs(res["row_freq"] - mean_pi)) <= 6 * np.sqrt(0.25 / S)  # row by row: a Bernoulli mean
    acc.close()
    pp.close()
    model.close()


def test_an_omitted_group_effect_is_flagged_and_the_full_design_is_not(la):
    """300 rows, logit = 0.4 x +- 1.5 by group: the design without the group puts both groups' observed counts in the tails of their
    replicates (two-sided p < 0.01); with the group in the design both one-sided p-values, p_ge and p_le, lie in [0.05, 0.95] (the
    two-sided value of a count the model reproduces is near 1)."""
    rng = np.random.default_rng(12)
    n, S = 300, 4000
    z = (np.arange(n) % 2).astype(np.float64)
    x = rng.standard_normal(n)
    y = (rng.random(n) < 1 / (1 + np.exp(-(0.4 * x + 1.5 * (2 * z - 1))))).astype(np.float64)
    groups = z.astype(np.int32)
    p_two, one_sided = {}, {}
    for name, X in (("omitted", np.stack([np.ones(n), x], axis=1)), ("full", np.stack([np.ones(n), x, z], axis=1))):
        sd = np.full(X.shape[1], 5.0)
        model = la.LogReg(X, y, sd, dtype="float32")
        acc = la.PredictiveCheck(model, groups=groups, seed=5)
        res = acc.update(laplace_draws(X, y, sd, S, 6)).result()
        p_two[name], one_sided[name] = res["p_two"], np.concatenate([res["p_ge"], res["p_le"]])
        note(f"[ppc] {name}: observed {res['t_obs'].tolist()}, replicated mean {np.round(res['mean'], 2).tolist()}, p_ge {res['p_ge'].tolist()}, p_le {res['p_le'].tolist()}, dev_p {res['dev_p']:.3f}")
        acc.close()
        model.close()
    assert np.all(p_two["omitted"] < 0.01) and np.all((one_sided["full"] >= 0.05) & (one_sided["full"] <= 0.95))
