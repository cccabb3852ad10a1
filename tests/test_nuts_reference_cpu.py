"""NUTS tree building against an independent reference, in the GPU-less container.

tests/nuts_reference.py restates one NUTS transition from DESIGN.md "NUTS" without the checkpoint scheme (stored leaf momenta, every
aligned span summed with math.fsum).  Here:
* the reference itself samples a correlated Gaussian correctly (callables, not the logistic model);
* the CPU test double (tests/host/lr_cpu_twin_nuts.c) equals it transition by transition, teacher-forced, at every padded width and
  both sides of each (p = 2 .. 32), unit and non-unit metrics, max_depth 1 .. 10, chain and iteration offsets (one beyond 2^32), with
  every way a tree can end occurring at least 20 times -- the count is asserted;
* `kernels._numpy_nuts` equals it on NumPy's global generator, drawn lazily in the order of the text;
* the float32 mode of the reference against its float64 mode over the GPU test's float32 cases: the measured decision margin and state
  deviation behind nuts_reference.F32_TAU / F32_STATE_TOL, and the share of transitions the margin excludes.
"""
import collections

import numpy as np
import pytest

import nuts_reference as nr
import twin_nuts


@pytest.fixture(scope="module", autouse=True)
def _nuts_twin():
    twin_nuts.install()
    yield
    twin_nuts.uninstall()


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


def test_reference_on_a_correlated_gaussian():
    """The reference guards nothing unless it is a correct sampler: 3000 transitions on N(0, [[1, .8], [.8, 1]]) through callables.
    Bound as test_generic_numpy_nuts_on_a_correlated_gaussian: the mean within 4 standard errors at a conservative ESS of a third
    of the draws (NUTS draws here are nearly independent), the covariance within 0.12 (its own standard error at that ESS is
    sqrt((1 + 0.64) / 933) = 0.042 for the off-diagonal and 0.046 for the diagonal: 0.12 is 2.6 of them)."""
    cov = np.array([[1.0, 0.8], [0.8, 1.0]])
    prec = np.linalg.inv(cov)
    np.random.seed(4)
    x, xs, reasons = np.zeros(2), [], collections.Counter()
    for _ in range(3000):
        t = nr.transition(lambda q: -0.5 * q @ prec @ q, lambda q: -prec @ q, x, 0.3, 1.0, 6, nr.NumpyStream(2))
        x = t.x
        xs.append(x)
        reasons[t.reason] += 1
    s = np.array(xs[200:])
    se = 1.0 / np.sqrt(len(s) / 3)
    print("reference on the Gaussian: mean", s.mean(axis=0), "cov", np.cov(s.T).round(3).tolist(), dict(reasons))
    assert np.all(np.abs(s.mean(axis=0)) < 4 * se)
    np.testing.assert_allclose(np.cov(s.T), cov, atol=0.12)


@pytest.fixture(scope="module")
def double_vs_reference(la):
    """every case of nr.CPU_CASES: the double's transitions and the reference's from the same inputs"""
    from oracle.oracle import OracleModel
    res = []
    for case in nr.CPU_CASES:
        X, y, ps = nr.synthetic_model(case.p, case.n, 100 + case.p)
        dmm, q0 = nr.case_metric_and_start(case)
        steps = nr.run_stepwise(la, la.LogReg(X, y, ps, dtype="float64"), q0, case.K, case.eps, dmm, case.max_depth, case.seed,
                                case.chain_offset, case.iter_offset)
        om = OracleModel(X, y, ps)
        refs = nr.reference_steps(om.lpost, om.glp, steps, case.eps, dmm, case.max_depth, case.seed, case.chain_offset, case.iter_offset)
        res.append((case, steps, refs))
    return res


def test_double_equals_the_reference_teacher_forced(double_vs_reference):
    """Every transition of the double from its own previous output against the reference from that same state and (seed, chain,
    iteration): signed depth, leaf count, divergence and max-depth flags equal; state and acceptance statistic within
    nr.F64_TOL = 8.3e-12 = 10 x the largest deviation measured here (8.24e-13, relative to the state's largest coordinate; the
    reference's exact sums against the double's fma chains over up to 1023 steps; profiles/r8_nuts_reference.txt).  Only a
    transition whose reference margin is below 1e-9 may be left out, and at most 1 in 1000 of them."""
    n = skipped = 0
    worst, mism = 0.0, []
    for case, steps, refs in double_vs_reference:
        cn, cs, cm, cw = nr.compare(steps, refs, nr.MIN_MARGIN)
        n, skipped, worst = n + cn, skipped + cs, max(worst, cw)
        mism += [f"{case}: {m}" for m in cm]
    print(f"double vs reference: {n} transitions, {skipped} skipped, largest relative deviation {worst:.3g}")
    assert not mism, "\n".join(mism[:20])
    assert skipped <= n / 1000
    assert worst <= nr.F64_TOL


def test_every_way_a_tree_ends_is_covered(double_vs_reference):
    """The comparison above only means something if the cases reach every decision: each stop reason at least 20 times, 'check 2
    only' and 'check 3 only' among them, and 20 subtree U-turns that only a span of 8 or more leaves shows."""
    cnt, widths, depths = collections.Counter(), collections.Counter(), collections.Counter()
    long_span = 0
    for case, steps, refs in double_vs_reference:
        for row in refs:
            for r in row:
                cnt[r.reason] += 1
                depths[abs(r.depth)] += 1
                widths[case.p] += 1
                long_span += r.reason == nr.SUBTREE and r.turn_span >= 8
    print("stop reasons:", dict(cnt), "| subtree U-turns at span >= 8:", long_span, "| depths:", sorted(depths.items()),
          "| transitions per p:", sorted(widths.items()))
    for reason in nr.REASONS:
        assert cnt[reason] >= 20, (reason, dict(cnt))
    assert long_span >= 20
    assert set(widths) == {2, 3, 4, 5, 8, 9, 15, 16, 17, 24, 31, 32}
    assert {c.max_depth for c, _, _ in double_vs_reference} == {1, 2, 3, 6, 10}
    assert any(c.iter_offset >= 2 ** 32 for c, _, _ in double_vs_reference) and all(c.n % 16 for c, _, _ in double_vs_reference)


def _lazy_pair(lpost, glp, x0, eps, dmm, md, iters, seed):
    """`iters` transitions of the generic kernel, each repeated by the reference from the same state and generator state"""
    import logreg_amd as la
    k = la.nutsKernel(lpost, glp, eps=eps, dmm=dmm, max_depth=md)
    assert not isinstance(k, la.FusedKernel)
    x, shapes, worst = np.asarray(x0, dtype=np.float64), collections.Counter(), 0.0
    for i in range(iters):
        np.random.seed(seed + i)
        a = k(x)
        after = np.random.get_state()[1:3]
        np.random.seed(seed + i)
        t = nr.transition(lpost, glp, x, eps, dmm, md, nr.NumpyStream(len(x)))
        # the same number of draws: the same leaves, subtrees and merges (each consumes its own)
        assert all(np.array_equal(u, v) for u, v in zip(after, np.random.get_state()[1:3])), (i, t)
        worst = max(worst, float(np.max(np.abs(a - t.x)) / max(np.max(np.abs(t.x)), 1e-300)))
        shapes[t.reason] += 1
        x = a
    return worst, shapes


def test_numpy_nuts_equals_the_reference():
    """`kernels._numpy_nuts` draws randn for the momentum, one rand per direction, one per leaf after a subtree's first and one per
    merge, in that order; NumpyStream gives the reference the same numbers when it asks in the order of the text.  Teacher-forced,
    300 transitions on the correlated Gaussian and 300 on a logistic model: the generic kernel returns the state only, so the tree's
    shape is compared through the generator -- both must have consumed the same number of draws -- and the state to nr.F64_TOL."""
    from oracle.oracle import OracleModel
    cov = np.array([[1.0, 0.8], [0.8, 1.0]])
    prec = np.linalg.inv(cov)
    worst, shapes = _lazy_pair(lambda q: -0.5 * q @ prec @ q, lambda q: -prec @ q, np.zeros(2), 0.3, np.array([1.0, 0.5]), 6, 300, 9)
    print("numpy NUTS on the Gaussian:", dict(shapes), "largest relative deviation", worst)
    assert worst <= nr.F64_TOL
    X, y, ps = nr.synthetic_model(5, 37, 105)
    om = OracleModel(X, y, ps)
    worst, shapes = _lazy_pair(om.lpost, om.glp, np.zeros(5), 0.25, np.array([0.5, 1.0, 2.0, 1.0, 0.7]), 7, 300, 1000)
    print("numpy NUTS on a logistic model:", dict(shapes), "largest relative deviation", worst)
    assert worst <= nr.F64_TOL
    assert shapes[nr.SUBTREE] >= 20 and shapes[nr.TREE] >= 20


def test_float32_mode_against_float64_sets_the_gpu_bounds():
    """The float32 kernel test's two numbers, from the reference alone: over nr.F32_CASES, teacher-forced along the float32 mode's
    own chain, the float64 mode from the float32-rounded data and state.  tau must be at least 8 x the largest float64 margin at
    which the two modes disagree (tree shape, flags or selected leaf), the state tolerance at least 8 x their largest relative
    deviation where they agree, and the transitions with a margin below tau at most 10 %.
    The 3096 transitions here see no disagreement (largest deviation 3.19e-05, no margin below tau); the constants come from the
    same cases at 330 chains under 48 seeds, `python tests/nuts_reference.py 48`: 2 disagreements in 380 160 transitions, the
    larger at a margin of 4.945e-07 (F32_TAU = 4.0e-6), largest deviation 2.04e-04 (F32_STATE_TOL = 1.64e-3), 0.010 % of the margins
    below F32_TAU (profiles/r8_nuts_reference.txt)."""
    m = nr.measure_float32_mode()
    print(f"float32 mode vs float64 mode: {m['n']} transitions, {m['disagree']} disagree, largest disagreeing margin {m['tau']:.3g}, "
          f"largest relative deviation {m['dev']:.3g}, share below F32_TAU {m['share']:.4f}")
    assert 8 * m["tau"] <= nr.F32_TAU
    assert 8 * m["dev"] <= nr.F32_STATE_TOL
    assert m["share"] <= 0.10
