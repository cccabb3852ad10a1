"""The cases of NUTS on the stepwise engine (logreg_amd/csrc/lr_tall_nuts.h) -- TEST INFRASTRUCTURE ONLY, a helper module of
tests/test_nuts_tall_cpu.py (which runs the reference alone over them, on the CPU) and tests/test_gpu_nuts_tall.py (the kernel against
the reference).  A case is a `nuts_reference.Case` on `nuts_reference.synthetic_model` plus the slice count asked of the planner.

Shapes: the smallest that reach each path of the kernel.  P lanes per chain in 256-lane blocks: p = 3, 8, 12, 17, 32 (P = 4, 8, 16, 32 and
a full 32), p = 33, 64 (P = 64: a chain fills one wave), p = 65, 128 (P = 128: a chain spans two waves, the sums go through LDS); 1, 3, 65
and 257 chains (part of a block, several blocks); row counts just beyond what the fused kernel's LDS holds (601 .. 3001: below that the stepwise mode is refused for
NUTS), in the planner's slices and in 1, 3 and 4 asked ones with a shorter last one; n = 100 for the wide widths; max_depth 10 with small steps (trees beyond depth 7: the second leaf-uniform block, deep checkpoints),
large steps from the tails (divergences and early stops beside building chains), max_depth 1 and 2, the high iteration word."""
import collections

import numpy as np

import nuts_reference as nr

TallCase = collections.namedtuple("TallCase", "case group")


def padded(p):
    return next(P for P in (4, 8, 16, 32, 64, 128) if p <= P)


# Rows per narrow width: just beyond what the fused kernel's LDS holds (rows + checkpoints at max_depth 10), the smallest the stepwise
# path accepts -- below it LR_MODE_STEPWISE is refused for NUTS, as it always was.  Steps scale with the posterior's width, ~ 1 / sqrt(n).
N_F64 = {3: 3001, 8: 2001, 12: 1001, 17: 601, 32: 601}
N_F32 = {3: 9001, 8: 5001, 17: 1501, 32: 1501}


def _f64_cases():
    cases = []
    for i, p in enumerate((3, 8, 17, 32)):
        n = N_F64[p]
        r = n ** -0.5
        C = (1, 3, 65, 257)[i]
        cases.append(TallCase(nr.Case(p, n, round(2.5 * r, 4), 6, i % 2 == 0, C, 6 if C <= 3 else 2, 600 + i, 3 + i, 5 + i, 1.0), (0, 3, 4, 1)[i]))  # asked slices
        cases.append(TallCase(nr.Case(p, n, round(2.0 * r, 4), 6, i % 2 == 1, (65, 257, 1, 3)[i], 2 if i < 2 else 6, 610 + i, 4 + i, 6, 1.0), (3, 0, 1, 4)[i]))
        cases.append(TallCase(nr.Case(p, n, round((0.004, 0.006, 0.012, 0.012)[i] * r, 6), 10, i % 2 == 1, 3, 3, 620 + i, 11 * i, 2 ** 32 * (i % 2) + i, 1.0), 0))  # deep
        cases.append(TallCase(nr.Case(p, n, round((8.0, 12.0)[i % 2] * r, 3), 10, i % 2 == 0, 65, 2, 630 + i, 1000 + i, 17, 3.0), 0))                   # tails
        cases.append(TallCase(nr.Case(p, n, round(1.5 * r, 4), 1 + i % 2, True, 8, 3, 640 + i, 7, 2 ** 20 + i, 1.0), 0))               # max_depth 1, 2
    cases.append(TallCase(nr.Case(12, N_F64[12], 0.0004, 10, True, 3, 2, 661, 129, 2 ** 33 + 1, 1.0), 0))  # P = 16, deep
    for i, p in enumerate((33, 64, 65, 128)):
        cases.append(TallCase(nr.Case(p, 100, 0.12, 6, i % 2 == 0, (65, 3, 257, 1)[i], (2, 6, 1, 6)[i], 670 + i, 4 * i, 2 + i, 1.0), 0))
        cases.append(TallCase(nr.Case(p, 100, (0.004, 0.004, 0.01, 0.012)[i], 10, i % 2 == 1, 3, 2, 680 + i, 65 * i, 2 ** 32 * (i % 2) + 3, 1.0), 0))  # deep
        cases.append(TallCase(nr.Case(p, 100, 0.9, 10, i % 2 == 0, 9, 2, 690 + i, 5, 1, 3.0), 0))                                              # tails
    return cases


F64_CASES = _f64_cases()
OFF_CHIP = TallCase(nr.Case(8, 20000, 0.02, 6, False, 64, 2, 700, 3, 1, 1.0), 0)  # the shape LR_MODE_AUTO refuses: rows beyond the LDS

# The float64 bound, per case.  nuts_reference.F64_TOL (8.3e-12) is 10 x the deviation between two summation orders over cases of at most 53
# rows, and it is the bound of every case here -- all wide ones, n = 20 000, every moderate and deep tree -- but three: the narrow cases of
# large steps from starts at 3 x the prior scale, where energies of 1e4 cancel.  On the MI355X those three exceeded F64_TOL (9.09e-11,
# 1.27e-11, 1.18e-11; every other case at most 6.4e-12, the wide ones 1.25e-12, n = 20 000 6.97e-13).  For a case that exceeds it the bound
# is made again as F64_TOL was, for that case alone and not from the kernel: the reference under slice-ordered float64 sums
# (SliceOrderModel below) against the reference itself on the CPU (`python tests/nuts_tall_cases.py order`; profiles/r23_nuts_tall.txt: no
# transition differs in shape), times 10.
F64_SLICE_DEV = {630: 9.823e-11,   # p = 3, n = 3001, eps 0.146
                 632: 6.821e-12,   # p = 17, n = 601, eps 0.326
                 633: 2.843e-11}   # p = 32, n = 601, eps 0.489


def f64_tol(tc):
    """the float64 bound of a case (keyed by its seed)"""
    return max(nr.F64_TOL, 10 * F64_SLICE_DEV[tc.case.seed]) if tc.case.seed in F64_SLICE_DEV else nr.F64_TOL


# float32: the narrow widths at row counts beyond the float32 LDS (moderate trees), and the wide ones
F32_NARROW = [TallCase(nr.Case(p, n, round(2.0 * n ** -0.5, 4), 10, i % 2 == 0, 33, 3, 710 + i, 7 * i, 3 + i, 1.0), 0) for i, (p, n) in enumerate(N_F32.items())]
F32_WIDE = [TallCase(nr.Case(p, 100, eps, 10, i % 2 == 0, 33, 3, 720 + i, 7 * i, 3 + i, 1.0), 0)
            for i, (p, eps) in enumerate(((33, 0.06), (64, 0.05), (65, 0.05), (128, 0.04)))]

# The float32 bounds of the wide cases: 8 x what the reference's NumPy-float32 mode showed against its float64 mode on the CPU over
# F32_WIDE widened to 330 chains under 8 seeds (`python tests/nuts_tall_cases.py`; profiles/r23_nuts_tall.txt), as nuts_reference.F32_TAU
# and F32_STATE_TOL were made for p <= 32; the larger of the two pairs holds for p > 32, the old pair alone for p <= 32.
F32_WIDE_TAU_MEASURED = 8.268e-08  # largest float64 margin at which the two modes disagreed (1 disagreement in 31 680 transitions, at p = 33)
F32_WIDE_DEV_MEASURED = 1.548e-04  # largest relative deviation where they agreed (at p = 64)
F32_WIDE_TAU = max(nr.F32_TAU, 8 * F32_WIDE_TAU_MEASURED)
F32_WIDE_STATE_TOL = max(nr.F32_STATE_TOL, 8 * F32_WIDE_DEV_MEASURED)


def problem(tc, dtype="float64"):
    """-> X, y, pscale, dmm, q0 of a case (float32: data and start rounded to float32, as nuts_reference.float32_problem)"""
    c = tc.case
    if dtype == "float32":
        return nr.float32_problem(c)
    X, y, ps = nr.synthetic_model(c.p, c.n, 100 + c.p)
    dmm, q0 = nr.case_metric_and_start(c)
    return X, y, ps, dmm, q0


def run_stepwise(la, model, q0, K, eps, dmm, max_depth, seed, chain_offset=0, iter_offset=0, group=0):
    """nuts_reference.run_stepwise on the stepwise engine: K iterations at thin 1, one call per iteration, each from the previous output"""
    k = la.nutsKernel(model.lpost, model.glp, eps=eps, dmm=dmm, max_depth=max_depth)
    x = np.ascontiguousarray(np.atleast_2d(q0), dtype=model.np_dtype)
    steps = []
    for it in range(K):
        cs = la.ChainSet(k, x, seed=seed, chain_offset=chain_offset, mode="stepwise", group=group)
        cs.iter_offset = iter_offset + it
        d = la.DeviceArray(model.device, (1, cs.C), np.int8)
        out = cs.advance(1, 1, depth=d).to_host()[0]
        cn = cs.get_counters()
        steps.append(dict(x_in=x, x_out=out, depth=d.to_host()[0].astype(int), **{f: np.array(cn[f]) for f in
                          ("n_leapfrog", "divergent", "max_depth_hits", "accept_stat_sum")}))
        x = out
    return steps


def kernel_vs_reference(la, tc, dtype="float64"):
    """-> steps of the kernel, the float64 reference's transitions from the kernel's own inputs"""
    from oracle.oracle import OracleModel
    c = tc.case
    X, y, ps, dmm, q0 = problem(tc, dtype)
    steps = run_stepwise(la, la.LogReg(X, y, ps, dtype=dtype), q0, c.K, c.eps, dmm, c.max_depth, c.seed, c.chain_offset, c.iter_offset, tc.group)
    om = OracleModel(X, y, ps)
    return steps, nr.reference_steps(om.lpost, om.glp, steps, c.eps, dmm, c.max_depth, c.seed, c.chain_offset, c.iter_offset)


def reference_free_running(tc):
    """the float64 reference alone over a case, each iteration from its own previous output -> its transitions, flat"""
    from oracle.oracle import OracleModel
    c = tc.case
    X, y, ps, dmm, q0 = problem(tc)
    om = OracleModel(X, y, ps)
    x, res = np.array(q0, dtype=np.float64), []
    for k in range(c.K):
        row = [nr.transition(om.lpost, om.glp, x[ch], c.eps, dmm, c.max_depth, nr.PhiloxStream(c.seed, c.chain_offset + ch, c.iter_offset + k, c.p))
               for ch in range(c.C)]
        res += row
        x = np.array([t.x for t in row])
    return res


def POSTERIOR_MODEL():
    """the tall model of the posterior test: n = 5001 x p = 8, rows beyond the LDS in both dtypes"""
    return nr.synthetic_model(8, 5001, 108)


def posterior_scales(X, y, ps):
    """-> MAP and Laplace standard deviations by Newton's method on the CPU oracle's float64 model (no GPU)"""
    from oracle.oracle import OracleModel
    om = OracleModel(X, y, ps)
    p = X.shape[1]
    b = np.zeros(p)
    for _ in range(50):
        w = 1.0 / (1.0 + np.exp(-X @ b))
        H = (X * (w * (1 - w))[:, None]).T @ X + np.diag(1.0 / np.broadcast_to(ps, (p,)) ** 2)
        step = np.linalg.solve(H, om.glp(b))
        b = b + step
        if np.max(np.abs(step)) < 1e-12:
            break
    return b, np.sqrt(np.diag(np.linalg.inv(H)))


class SliceOrderModel:
    """The model in float64 with every sum over the rows taken slice by slice, left to right inside a slice and over the slices (the
    order of the stepwise engine's reduction, as plain NumPy): a second summation order for the reference to be measured under."""

    def __init__(self, X, y, pscale, slices):
        self.X, self.sign, self.y = np.asarray(X, dtype=np.float64), 2.0 * np.asarray(y, dtype=np.float64) - 1.0, np.asarray(y, dtype=np.float64)
        n, p = self.X.shape
        ps = np.broadcast_to(np.asarray(pscale, dtype=np.float64), (p,))
        self.inv_var = 1.0 / (ps * ps)
        self.lprior_const = float(np.sum(-0.5 * np.log(2.0 * np.pi) - np.log(ps)))
        ln = -(-n // max(1, slices))
        self.bounds = [(a, min(n, a + ln)) for a in range(0, n, ln)]

    def _eta(self, q):
        return np.cumsum(self.X * np.asarray(q, dtype=np.float64), axis=1)[:, -1]

    def lpost(self, q):
        with np.errstate(over="ignore", invalid="ignore"):
            t = -np.logaddexp(0.0, -self.sign * self._eta(q))
            ll = 0.0
            for a, b in self.bounds:
                ll += float(np.cumsum(t[a:b])[-1])
            q = np.asarray(q, dtype=np.float64)
            return ll + self.lprior_const - 0.5 * float(np.cumsum(q * q * self.inv_var)[-1])

    def glp(self, q):
        with np.errstate(over="ignore", invalid="ignore"):
            r = self.y - 1.0 / (1.0 + np.exp(-self._eta(q)))
            g = np.zeros(self.X.shape[1])
            for a, b in self.bounds:
                g = g + np.cumsum(self.X[a:b] * r[a:b, None], axis=0)[-1]
            return g - np.asarray(q, dtype=np.float64) * self.inv_var


def measure_slice_order(cases=None):
    """The reference under the slice-ordered sums against the reference itself, teacher-forced along the latter's chain: -> list of
    (case, transitions, transitions whose shape differs, largest relative deviation of state or acceptance statistic among the others --
    nuts_reference.compare's measure)."""
    from oracle.oracle import OracleModel
    res = []
    for t in cases or F64_CASES + [OFF_CHIP]:
        c = t.case
        X, y, ps, dmm, q0 = problem(t)
        om, sm = OracleModel(X, y, ps), SliceOrderModel(X, y, ps, t.group or max(1, c.n // 256))
        x, n, differ, dev = np.array(q0, dtype=np.float64), 0, 0, 0.0
        for k in range(c.K):
            nxt = []
            for ch in range(c.C):
                args = (c.eps, dmm, c.max_depth, nr.PhiloxStream(c.seed, c.chain_offset + ch, c.iter_offset + k, c.p))
                a, b = nr.transition(om.lpost, om.glp, x[ch], *args), nr.transition(sm.lpost, sm.glp, x[ch], *args)
                nxt.append(a.x)
                n += 1
                if nr.shape_of(a) != nr.shape_of(b) or a.prop_leaf != b.prop_leaf:
                    differ += 1
                elif not np.isnan(a.x).any():
                    d = float(np.max(np.abs(a.x - b.x)) / max(np.max(np.abs(a.x)), 1e-300))
                    if a.accept_stat > 0:
                        d = max(d, abs(a.accept_stat - b.accept_stat) / a.accept_stat)
                    dev = max(dev, d)
            x = np.array(nxt)
        res.append((t, n, differ, dev))
    return res


def _measure(case):
    return nr.measure_float32_mode([case])


def _measure_order(t):
    return measure_slice_order([t])[0]


if __name__ == "__main__":
    # python tests/nuts_tall_cases.py [replicates]: the float32 measurement behind F32_WIDE_TAU / F32_WIDE_STATE_TOL
    import multiprocessing
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    if sys.argv[1:2] == ["order"]:  # python tests/nuts_tall_cases.py order: the measurement behind F64_SLICE_DEV
        with multiprocessing.Pool(16) as pool:
            res = pool.map(_measure_order, F64_CASES + [OFF_CHIP], chunksize=1)
        for t, n, differ, dev in res:
            print(f"{t}: {n} transitions, {differ} differ in shape, largest relative deviation {dev:.4g}")
        worst = max(r[3] for r in res)
        print(f"all: {sum(r[1] for r in res)} transitions, {sum(r[2] for r in res)} differ in shape; largest relative deviation {worst:.4g} (x 10 = {10 * worst:.4g})")
        sys.exit(0)
    if sys.argv[1:2] == ["posterior"]:  # python tests/nuts_tall_cases.py posterior: writes tests/golden/nuts_tall_posterior.json
        import json
        from logreg_amd.diagnostics import summarise
        from oracle.oracle import OracleModel, max_threads
        X, y, ps = POSTERIOR_MODEL()
        om = OracleModel(X, y, ps)
        beta, sd = posterior_scales(X, y, ps)
        q0 = beta + sd * np.random.default_rng(1).standard_normal((256, X.shape[1]))
        runs = {}
        # the CPU oracle's HMC (float64, its own code) under the Laplace-scale diagonal metric; trajectory length L x eps below the quarter
        # period pi / 2 of a nearly Gaussian target in these units, where a fixed-length trajectory cannot resonate; two settings must agree
        for name, (eps, L) in {"main": (0.3, 5), "check": (0.35, 3)}.items():
            r = om.run("hmc", q0, step=eps, l=L, scale=1 / sd ** 2, thin=100, iters=1, seed=11, threads=min(16, max_threads()))
            r = om.run("hmc", r["state"], step=eps, l=L, scale=1 / sd ** 2, thin=2, iters=400, seed=11, iter_offset=100, threads=min(16, max_threads()))
            sm = summarise(r["out"], max_chains=256)
            runs[name] = {k: np.asarray(v).tolist() for k, v in sm.items()}
            runs[name]["se_sd"] = (sm["sd"] / np.sqrt(2 * sm["ess"])).tolist()
            runs[name]["accept"] = float(r["accepts"].mean() / 800)
            print(name, "sd / Laplace", np.round(sm["sd"] / sd, 4), "ess", np.round(sm["ess"]), "accept", runs[name]["accept"])
        a, b = runs["main"], runs["check"]
        z = (np.array(a["mean"]) - np.array(b["mean"])) / np.hypot(a["mcse"], b["mcse"])
        zs = (np.array(a["sd"]) - np.array(b["sd"])) / np.hypot(a["se_sd"], b["se_sd"])
        print("main against check: z(mean)", np.round(z, 2), "z(sd)", np.round(zs, 2))
        assert np.max(np.abs(z)) < 4.2 and np.max(np.abs(zs)) < 4.2
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nuts_tall_posterior.json"), "w") as f:
            json.dump({"source": "oracle.OracleModel.run('hmc') on nuts_reference.synthetic_model(8, 5001, 108): 256 chains, 100 iterations discarded, "
                                 "400 kept at thin 2, eps 0.3 x L 5 under dmm = 1 / (Laplace sd)^2 (python tests/nuts_tall_cases.py posterior)",
                       "pooled": a, "check_eps0.35_L3": b, "map": beta.tolist(), "laplace_sd": sd.tolist()}, f, indent=1)
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    todo = [tc.case._replace(C=330, seed=tc.case.seed + 1000 * r) for r in range(reps) for tc in (F32_NARROW if sys.argv[2:3] == ["narrow"] else F32_WIDE)]
    with multiprocessing.Pool(16) as pool:
        res = pool.map(_measure, todo, chunksize=1)
    for p_ in sorted({c.p for c in todo}):
        sel = [m for c, m in zip(todo, res) if c.p == p_]
        print(f"p={p_}: {sum(m['n'] for m in sel)} transitions, {sum(m['disagree'] for m in sel)} disagree, largest disagreeing margin "
              f"{max(m['tau'] for m in sel):.4g}, largest relative deviation {max(m['dev'] for m in sel):.4g}")
    tau, dev = max(m["tau"] for m in res), max(m["dev"] for m in res)
    mg = np.concatenate([m["margins"] for m in res])
    print(f"all: {len(mg)} transitions; largest disagreeing margin {tau:.4g} (x 8 = {8 * tau:.4g}); largest relative deviation {dev:.4g} "
          f"(x 8 = {8 * dev:.4g}); share of margins below nr.F32_TAU = {nr.F32_TAU:g}: {np.mean(mg < nr.F32_TAU):.5f}")
