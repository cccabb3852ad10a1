"""Cases and fixture generator of tests/test_gpu_stepwise_parent.py: every launch sequence of the stepwise engine (lr_engine.h, as
lr_plan.h plan_stepwise lays it out) at the smallest shapes that take it, 70 chains (one sequence needs 1024) and 3 iterations each.  Results are compared BYTE FOR
BYTE with a recording made on another build:

    python tests/stepwise_parent_cases.py --write tests/golden/stepwise_parent.json --commit <id of the recorded build's commit>

run once, on the GPU, in a checkout of that commit (this file copied into its tests/).  Every array is recorded as the SHA-256 of its
bytes; the recording also holds the device's CU count, since the plans depend on it.

HMC with L leapfrog steps has L - 1 interior steps.  On the fused row-split kernels (wide: wide_traj=0; tall: the 16-wave kernel) L = 2 is
one launch with no fused prologue, L = 3 swaps the two buffer pairs once, L = 4 twice: the smallest sequences at which a launch that read
the wrong pair, summed the wrong number of slice partials or took float32 partials for float64 ones would show.  The float64 models are
the runs whose update reads float32 partials, once per step (n = 2600: more slices than the prologue sums) and once after a fused hand-over.
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(REPO, "tests", "golden", "stepwise_parent.json")
SEED, C, ITERS = 20271, 70, 3

# (n, p, LOGREG_DEBUG_OPTS): wide on the trajectory kernel (one tile, forced two tiles), on the fused and on the per-step row-split kernel, on
# the bf16 operand format; tall on the 4-wave interior kernel (with so few chains, whatever tall_mx16 says: TALL_FUSED below); 17 <= p <= 32
SHAPES = [(900, 128, ""), (900, 128, "wide_traj=0"), (900, 128, "wide_traj=2"), (2600, 128, "wide_traj=0"), (900, 128, "wide_f16=0"), (3000, 8, ""),
          (3000, 8, "tall_mx16=0"), (1500, 20, "")]
SHAPES_F64 = [(900, 128, "wide_traj=0"), (2600, 128, "wide_traj=0"), (3000, 8, "")]
# (dtype, n, p, options, L, precision)
HMC = ([("float32", n, p, opt, L, "auto") for n, p, opt in SHAPES for L in (1, 2, 3, 4)] +
       [("float64", n, p, opt, L, "auto") for n, p, opt in SHAPES_F64 for L in (2, 3, 4)] +
       [("float32", n, p, "", 4, prec) for n, p in ((900, 128), (3000, 8)) for prec in ("full", "bf16")])
MODELS = sorted({c[:4] for c in HMC})
OTHER = [(3000, 8), (300, 100)]  # RWMH, MALA, UL, the four closures, NUTS
NUTS_TALL = (6000, 8)            # (NUTS takes the stepwise engine only where the fused kernel cannot hold the rows: refused at n = 3000)
# The tall 16-wave interior kernel with its fused prologue needs slices of 1024 rows that still fill three quarters of the chip (lr_plan.h
# plan_interior): 16 slices x 16 chain blocks at 256 CUs -- the one sequence 70 chains cannot reach.  Both dtypes, L = 2, 3, 4.
TALL_FUSED = (16384, 8, 1024)


def data(n, p):
    """A small synthetic logistic regression, from NumPy's PCG64 streams only."""
    rng = np.random.default_rng(1000 * n + p)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    beta = rng.standard_normal(p) * 0.4 / np.sqrt(p)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return X, y, np.linspace(1.0, 3.0, p), np.linspace(0.5, 2.0, p)  # (a different prior and mass in every coordinate)


def init(n, p, chains=C):
    return (0.3 / np.sqrt(n)) * np.random.default_rng(7 * n + 31 * p + chains).standard_normal((chains, p))


@contextlib.contextmanager
def model(la, n, p, opt="", dtype="float32"):
    """A model created under LOGREG_DEBUG_OPTS = opt (read once, at creation)"""
    old = os.environ.get("LOGREG_DEBUG_OPTS")
    os.environ["LOGREG_DEBUG_OPTS"] = opt
    try:
        X, y, pscale, scale = data(n, p)
        m = la.LogReg(X, y, pscale, dtype=dtype)
    finally:
        if old is None:
            del os.environ["LOGREG_DEBUG_OPTS"]
        else:
            os.environ["LOGREG_DEBUG_OPTS"] = old
    try:
        yield m, scale
    finally:
        m.close()


def digest(**arrays):
    rec = {}
    for name, arr in arrays.items():
        arr = np.ascontiguousarray(arr)
        rec[name] = {"dtype": str(arr.dtype), "shape": list(arr.shape), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}
    return rec


def run(la, k, q0, thin=1, stats=False, lp=False, **kw):
    """One chain set on the stepwise engine, ITERS kept draws -> the digests of everything it hands back"""
    cs = la.ChainSet(k, q0, seed=SEED, mode="stepwise", **kw)
    assert cs.plan()["mode"] == "stepwise"
    if stats:
        cs.enable_stats(1, ITERS)
    nuts = k.kind == "nuts"
    depth = la.DeviceArray(k.model.device, (ITERS, cs.C), np.int8) if nuts else None
    out = cs.advance(ITERS, thin, depth=depth).to_host()
    cs.sync()
    rec = digest(samples=out, state=cs.state.to_host(), accepts=cs.get_accepts())
    if lp:
        rec.update(digest(lp=cs.get_ll()))
    if nuts:
        rec.update(digest(counters=cs.get_counters(), depth=depth.to_host()))
    if stats:
        rec.update(digest(stats=cs.stats.to_host()))
    return rec


def hmc(la, m, scale, L):
    return la.hmcKernel(m.lpost, m.glp, eps=0.4 / np.sqrt(m.n), l=L, dmm=scale)


def run_hmc_model(la, dtype, n, p, opt):
    """-> {case id: record} of every (L, precision) of one model"""
    res = {}
    with model(la, n, p, opt, dtype) as (m, scale):
        for d, nn, pp, oo, L, prec in HMC:
            if (d, nn, pp, oo) == (dtype, n, p, opt):
                res[f"hmc-{dtype}-n{n}-p{p}-[{opt}]-L{L}-{prec}"] = run(la, hmc(la, m, scale, L), init(n, p), precision=prec)
    return res


def run_other(la, n, p):
    res = {}
    with model(la, n, p) as (m, scale):
        sc = 1.0 / np.sqrt(n)
        q0 = init(n, p)
        tag = f"f32-n{n}-p{p}"
        res[f"rwmh-{tag}"] = run(la, la.mhKernel(m.lpost, la.rwProposal(0.3 * sc * scale)), q0, lp=True)
        res[f"mala-{tag}"] = run(la, la.malaKernel(m.lpost, m.glp, dt=0.05 * sc * sc, pre=scale), q0, lp=True)
        res[f"ul-{tag}"] = run(la, la.ulKernel(m.glp, dt=0.05 * sc * sc, pre=scale), q0)
        res[f"eval-{tag}"] = digest(**m.eval(q0, mode="stepwise"))
    return res


def run_nuts(la, n, p):
    """-> the record, or {"refused": True} where the planner keeps NUTS on the fused kernel"""
    with model(la, n, p) as (m, scale):
        k = la.nutsKernel(m.lpost, m.glp, eps=0.4 / np.sqrt(n), dmm=scale, max_depth=3)
        try:
            return {f"nuts-f32-n{n}-p{p}": run(la, k, init(n, p))}
        except la.LogregHipError:
            return {f"nuts-f32-n{n}-p{p}": {"refused": True}}


def run_tall_fused(la, dtype):
    n, p, chains = TALL_FUSED
    res = {}
    with model(la, n, p, "", dtype) as (m, scale):
        for L in (2, 3, 4):
            res[f"hmc-{dtype}-n{n}-p{p}-C{chains}-L{L}-auto"] = run(la, hmc(la, m, scale, L), init(n, p, chains))
    return res


def run_stats_and_shards(la):
    res = {}
    with model(la, 3000, 8) as (m, scale):  # streaming statistics, thin = 2
        res["hmc-f32-n3000-p8-L3-stats-thin2"] = run(la, hmc(la, m, scale, 3), init(3000, 8), thin=2, stats=True)
    with model(la, 900, 128, "wide_traj=0") as (m, scale):  # two shards of one run: each plans as the whole run does
        q0 = init(900, 128)
        for lo, hi in ((0, 35), (35, C)):
            res[f"hmc-f32-n900-p128-[wide_traj=0]-L4-shard{lo}"] = run(la, hmc(la, m, scale, 4), q0[lo:hi], chain_offset=lo, plan_chains=C, plan_first=0)
    return res


def device_cus(la):
    with model(la, 50, 4) as (m, _):
        return int(m._L.lr_device_cus(m.device))


def run_all(la):
    res = {}
    for dtype, n, p, opt in MODELS:
        res.update(run_hmc_model(la, dtype, n, p, opt))
    for n, p in OTHER + [NUTS_TALL]:
        if (n, p) != NUTS_TALL:
            res.update(run_other(la, n, p))
        res.update(run_nuts(la, n, p))
    for dtype in ("float32", "float64"):
        res.update(run_tall_fused(la, dtype))
    res.update(run_stats_and_shards(la))
    return res


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True)
    ap.add_argument("--commit", required=True, help="id of the commit whose build is being recorded")
    a = ap.parse_args()
    import logreg_amd
    from logreg_amd import build as lib_build
    doc = {"recorded_from_commit": a.commit, "library_build_id": lib_build.built_id(), "cus": device_cus(logreg_amd), "cases": run_all(logreg_amd)}
    os.makedirs(os.path.dirname(os.path.abspath(a.write)), exist_ok=True)
    with open(a.write, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases -> {a.write} ({os.path.getsize(a.write)} bytes)")
