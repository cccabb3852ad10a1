"""The model evaluation at saturated logits, on every engine (cases: tests/eval_cases.py; reference and bounds:
tests/eval_reference.py; both are checked without a GPU by tests/test_eval_regimes_cpu.py).

The device implementations of ll / lprior / lpost / glp differ from one another in one place: what happens when |t_i| = |xs_i . beta| is
large -- the clamps (100 in log2 units in the float32 row-pair and matrix-core forms, -750 in the float64 one-exponential form), the
overflow fall-back of the per-lane product form, the sigma(-t) select, the cancellation in ts - log2(1 + 2^ts) and the -log 2 per padded
row.  Every case holds 65 parameter vectors from max |t_i| = 1 to 5000 in one launch, so one wave mixes the regimes.

  (a) lr_eval on every engine that takes the shape, both dtypes, four `want` subsets (value only, gradient only and combined are different
      instantiations): all outputs within the bounds, finite, ll <= 0.  lr_eval reads a forced matrix-core or stepwise mode of a narrow
      model as the planner's choice (include/logreg_hip.h), so those two engines' own value and gradient paths are reached by (b) and (c).
  (b) the chain kernels' own value path: one RWMH iteration with a zero proposal scale from lp = -inf accepts, leaves the state as it
      was to the byte and writes lpost(state) to lp_state.  Every request lr_plan accepts must run, on the engine lr_plan named.
  (c) the chain kernels' gradient path: one unadjusted Langevin iteration against the oracle, whose glp form is overflow-safe.
  (d) lr_hessian across the 64-row blocks of its kernel, p up to its largest LDS request.

Nothing here is fitted to the kernels: the bounds come from the inputs (eval_reference.bounds), with three terms derived from the arithmetic
and named where they enter: the padded rows of the register layouts (ll), the prior's 1 / sd^2 on the Hessian's diagonal, the device's
normal draw in the Langevin step.  The largest error / bound ratios per engine
are printed when the module finishes (`pytest -s`; profiles/r22_eval_regimes.txt).
"""
import faulthandler
import os

import numpy as np
import pytest

import eval_cases as ec
import eval_reference as er

pytestmark = pytest.mark.gpu
C = ec.CHAINS
WANTS = (er.WANT, ("ll",), ("glp",), ("lpost", "glp"))
U32 = er.U["float32"]
_REF, _TOL, _MODELS, RATIOS = {}, {}, {}, {}


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
    print("\nlargest error / bound per section, dtype and planned engine")
    for key in sorted(RATIOS):
        print("  %-8s %-8s %-22s " % key + "  ".join(f"{k} {v:.3f}" for k, v in RATIOS[key].items()))


def reference(name, dtype, plan=None):
    """The reference of a case and its bounds for an engine (plan: register-resident rows carry the padding term of eval_reference.bounds)."""
    if (name, dtype) not in _REF:
        c = ec.case(name)
        _REF[(name, dtype)] = er.reference(c["X"], c["y"], c["prior_sd"], c["beta"], dtype)
    ref = _REF[(name, dtype)]
    pad = plan["group"] * plan["rows_per_lane"] - ec.case(name)["n"] if plan is not None and plan["mode"] == "reg" else 0
    assert pad >= 0
    if (name, dtype, pad) not in _TOL:
        _TOL[(name, dtype, pad)] = er.bounds(ref, dtype, pad)
    return ref, _TOL[(name, dtype, pad)]


def model(la, name, dtype, opts=""):
    """One model per case, dtype and LOGREG_DEBUG_OPTS value (the library reads the variable once, when the model is created)."""
    if (name, dtype, opts) not in _MODELS:
        c = ec.case(name)
        saved = os.environ.get("LOGREG_DEBUG_OPTS")
        try:
            if opts:
                os.environ["LOGREG_DEBUG_OPTS"] = opts
            m = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
        finally:
            if opts:
                if saved is None:
                    del os.environ["LOGREG_DEBUG_OPTS"]
                else:
                    os.environ["LOGREG_DEBUG_OPTS"] = saved
        assert ("wide_waves=8" in m.debug_opts()) == bool(opts)
        _MODELS[(name, dtype, opts)] = m
    return _MODELS[(name, dtype, opts)]


def requests(dtype, p):
    """(LOGREG_DEBUG_OPTS, mode, group) to try, as tests/fuzz_parity.py builds its engine list."""
    if p > 32:
        return [("", "auto", 0), ("wide_waves=8", "auto", 0)]
    if dtype == "float32":
        pairs = [("auto", 0)] + [("reg", g) for g in (16, 32, 64)] + [("lds", g) for g in (1, 8, 64)] + [("global", 1), ("global", 64)] + \
                [("mfma", 1), ("mfma", 4), ("stepwise", 0), ("stepwise", 3)]
    else:
        pairs = [("auto", 0)] + [("lds", g) for g in (1, 8, 16, 64)] + [("global", g) for g in (1, 16, 64)] + [("stepwise", 0), ("stepwise", 3)]
    return [("",) + q for q in pairs]


def engines(la, name, dtype):
    """[(model, mode, group, plan, label)]: every request of the list that lr_plan accepts for this case."""
    out = []
    for opts, mode, group in requests(dtype, ec.case(name)["p"]):
        m = model(la, name, dtype, opts)
        try:
            plan = m.plan(C, group, mode)
        except la.LogregHipError:
            continue  # no such variant for the shape
        out.append((m, mode, group, plan, "%s g%d r%d%s" % (plan["mode"], plan["group"], plan["rows_per_lane"], " ww8" if opts else "")))
    return out


def stop_on_hip_error(e):
    """A HIP runtime error (LR_ERR_HIP, -2) ends the whole run: nothing more is started on a device that has faulted."""
    if "error -2" in str(e):
        pytest.exit("HIP runtime error: " + str(e), returncode=3)


def note(section, dtype, label, rt):
    have = RATIOS.setdefault((section, dtype, label), {})
    for k, v in rt.items():
        have[k] = max(have.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------
def test_every_engine_is_reached_by_some_case(la):
    """The engine lists the tests below run are not silently empty: over the cases, the planned (dtype, mode) pairs contain every
    engine, each wide shape in both dtypes and both value forms of the register kernels (from 8 rows per lane the per-lane product)."""
    seen, reg_rows, wide = set(), set(), set()
    for name in ec.NAMES:
        c = ec.case(name)
        for dtype in ec.DTYPES:
            for m, mode, group, plan, label in engines(la, name, dtype):
                seen.add((dtype, plan["mode"]))
                if plan["mode"] == "reg":
                    reg_rows.add(plan["rows_per_lane"] >= 8)
                if c["p"] > 32:
                    assert plan["mode"] == "stepwise"
                    wide.add((dtype, c["p"], c["n"], "ww8" in label))
    assert {("float32", k) for k in ("reg", "lds", "global", "mfma", "stepwise")} <= seen, seen
    assert {("float64", k) for k in ("lds", "global", "stepwise")} <= seen, seen
    assert reg_rows == {True, False}
    assert wide == {(d, p, n, w) for d in ec.DTYPES for p, n in ec.SHAPES if p > 32 for w in (False, True)}


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("name", ec.NAMES)
def test_lr_eval_within_the_bounds_on_every_engine(la, name, dtype):
    c = ec.case(name)
    todo = engines(la, name, dtype)
    assert todo
    bad = []
    for m, mode, group, plan, label in todo:
        # (a forced matrix-core or stepwise mode is read as the planner's choice: the bounds are those of the kernel that runs)
        if mode in ("mfma", "stepwise") and c["p"] <= 32:
            plan = m.plan(C)
            label = "%s/%d as %s g%d r%d" % (mode, group, plan["mode"], plan["group"], plan["rows_per_lane"])
        ref, tol = reference(name, dtype, plan)
        for want in WANTS:
            try:
                got = m.eval(c["beta"], want, group=group, mode=mode)
            except la.LogregHipError as e:  # (a failure: lr_plan took the request)
                stop_on_hip_error(e)
                raise
            rt = er.ratios(got, ref, tol, want)
            note("eval", dtype, label, rt)
            for k in want:
                if not np.all(np.isfinite(got[k])):
                    bad.append((label, want, k, "not finite"))
                elif rt[k] > 1.0:
                    ch = int(np.argmax(np.max(np.abs(got[k] - ref[k]) / tol[k], axis=-1) if k == "glp" else np.abs(got[k] - ref[k]) / tol[k]))
                    bad.append((label, want, k, round(rt[k], 3), "chain %d" % ch, c["pairs"][ch]))
            if "ll" in want and np.any(got["ll"] > 0):
                bad.append((label, want, "ll > 0", float(np.max(got["ll"]))))
    print(name, dtype, "eval:", {label: {k: round(v, 3) for k, v in RATIOS[("eval", dtype, label)].items()} for *_, label in todo if ("eval", dtype, label) in RATIOS})
    assert not bad, bad


def one_iteration(la, kernel, beta, mode, group):
    """(states before and after one iteration, accepts, lp_state, plan, its label), or None where the library refuses the run."""
    try:
        cs = la.ChainSet(kernel, beta, seed=22, mode=mode, group=group, precision="full")
        plan = cs.plan()
        first = cs.state.to_host()
        out = cs.advance(1, 1).to_host()[0]
    except la.LogregHipError as e:
        stop_on_hip_error(e)
        return None
    return first, out, cs.get_accepts(), cs.get_ll(), plan, "%s g%d r%d" % (plan["mode"], plan["group"], plan["rows_per_lane"])


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("name", ec.NAMES)
def test_chain_kernels_value_path(la, name, dtype):
    """RWMH with prop_sd = 0 from lp = -inf: the proposal is the state, it is accepted, and lp_state becomes the kernel's own lpost(state)."""
    c = ec.case(name)
    bad = []
    for m, mode, group, planned, _ in engines(la, name, dtype):
        ref, tol = reference(name, dtype, planned)
        r = one_iteration(la, la.mhKernel(m.lpost, la.rwProposal(np.zeros(c["p"]))), c["beta"], mode, group)
        if r is None or r[4]["mode"] != planned["mode"]:
            bad.append((mode, group, planned, "no such run kernel" if r is None else r[4]))
            continue
        first, out, acc, lp, plan, label = r
        label += " ww8" if "wide_waves=8" in m.debug_opts() else ""
        q = np.abs(lp - ref["lpost"]) / tol["lpost"]
        note("rwmh", dtype, label, {"lpost": float(np.max(q)) if np.all(np.isfinite(lp)) else float("inf")})
        if not np.all(acc == 1):
            bad.append((label, "accepts", acc.tolist()))
        if first.tobytes() != out.tobytes() or first.dtype != out.dtype:
            bad.append((label, "state changed"))
        if not np.all(q <= 1.0):
            bad.append((label, "lp_state", float(np.max(q)), c["pairs"][int(np.argmax(q))]))
    print(name, dtype, "rwmh:", {k[2]: v for k, v in RATIOS.items() if k[0] == "rwmh" and k[1] == dtype})
    assert not bad, bad


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("name", ec.NAMES)
def test_chain_kernels_gradient_path(la, name, dtype):
    """One unadjusted Langevin iteration, x' = x + a glp(x) + b z with a_j = pre_j dt / 2, b_j = sqrt(pre_j dt), against the oracle on the
    data the model holds.  dt = 1 and pre is chosen per coordinate so that the gradient term shows in the new state of every chain:
    a_j sum_i |x_ij| = 200 u max_c |beta_cj| (a column of zeros: a_j / sd_j^2 = 200 u, the prior's pull), u = 2^-24 for both dtypes.
    Tolerance per coordinate: a_j tol_g[j] + 4 u |beta_j| + 4 u |b_j z_j| + b_j dz.
    The last term is the device's normal draw itself, which a bound relative to |z_j| knows nothing of where z_j is small (it shows at the
    intercept chains, whose other coordinates are zero and leave no other slack): float32 kernels compute Box-Muller on the hardware
    transcendentals, within dz = 4e-6 of the oracle's normals (test_device_normals_against_the_oracle holds them to it); float64 kernels
    round the angle 2 pi u2 once or twice, |d theta| <= 4 pi u, under a radius of at most sqrt(2 log 2^25) < 6: dz = 24 pi u."""
    from oracle import oracle as orc_mod
    c = ec.case(name)
    ref, tol = reference(name, dtype)
    u = er.U[dtype]
    colsum = np.abs(ref["xs"]).sum(axis=0)
    bmax = np.abs(ref["beta"]).max(axis=0)
    a = np.where(colsum > 0, 200 * U32 * np.maximum(bmax, 1e-30) / np.where(colsum > 0, colsum, 1.0), 200 * U32 * c["prior_sd"] ** 2)
    assert np.all(a[colsum > 0] * colsum[colsum > 0] >= 100 * U32 * bmax[colsum > 0])
    pre = 2.0 * a
    orc = orc_mod.OracleModel(er.held(c["X"], dtype), c["y"], c["prior_sd"])
    want = orc.run("ul", ref["beta"], step=1.0, scale=pre, thin=1, iters=1, seed=22, threads=0)["out"][0]
    assert np.all(np.isfinite(want))
    z = np.array([orc_mod.draws(22, ch, 0, c["p"])[0] for ch in range(C)])
    bz = np.abs(np.sqrt(pre)[None, :] * z)
    dz = 4e-6 if dtype == "float32" else 24 * np.pi * u
    bound = a[None, :] * tol["glp"] + 4 * u * np.abs(ref["beta"]) + 4 * u * bz + np.sqrt(pre)[None, :] * dz
    bad = []
    for m, mode, group, planned, _ in engines(la, name, dtype):
        r = one_iteration(la, la.ulKernel(m.glp, dt=1.0, pre=pre), c["beta"], mode, group)
        if r is None or r[4]["mode"] != planned["mode"]:
            bad.append((mode, group, planned, "no such run kernel" if r is None else r[4]))
            continue
        first, out, acc, _, plan, label = r
        label += " ww8" if "wide_waves=8" in m.debug_opts() else ""
        assert np.array_equal(first.astype(np.float64), ref["beta"])
        q = np.abs(out.astype(np.float64) - want) / bound
        note("ul", dtype, label, {"state": float(np.max(q)) if np.all(np.isfinite(out)) else float("inf")})
        if not np.all(q <= 1.0):
            ch, j = np.unravel_index(int(np.argmax(q)), q.shape)
            bad.append((label, float(np.max(q)), "chain %d coordinate %d" % (ch, j), c["pairs"][ch]))
    print(name, dtype, "ul:", {k[2]: v for k, v in RATIOS.items() if k[0] == "ul" and k[1] == dtype})
    assert not bad, bad


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("name", ec.HESS_NAMES)
def test_lr_hessian_within_the_bounds(la, name, dtype):
    """H within tol_H, symmetric to the bit, positive on the diagonal; grad and lpost within the float64 bounds (lr_hessian computes in
    float64 on the rows the model holds, with the caller's float64 beta)."""
    c = ec.hessian_case(name)
    ref = er.reference(c["X"], c["y"], c["prior_sd"], c["beta"], dtype, hessian=True, round_beta=False)
    tol = er.bounds(ref, "float64")
    tol_h = er.bound_hessian(ref)
    m = la.LogReg(c["X"], c["y"], c["prior_sd"], dtype=dtype)
    worst = {"H": 0.0, "glp": 0.0, "lpost": 0.0}
    for k, b in enumerate(c["beta"]):
        try:
            lp, g, H = m.hessian(b)
        except la.LogregHipError as e:
            stop_on_hip_error(e)
            raise
        assert np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(lp)
        assert np.array_equal(H, H.T) and np.all(np.diag(H) > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            qh = np.where(H == ref["H"][k], 0.0, np.abs(H - ref["H"][k]) / tol_h[k])
        worst["H"] = max(worst["H"], float(np.max(qh)))
        worst["glp"] = max(worst["glp"], float(np.max(np.abs(g - ref["glp"][k]) / tol["glp"][k])))
        worst["lpost"] = max(worst["lpost"], float(abs(lp - ref["lpost"][k]) / tol["lpost"][k]))
    note("hessian", dtype, "p%d" % c["p"], worst)
    print(name, dtype, "hessian:", worst)
    m.close()
    assert max(worst.values()) <= 1.0, worst
