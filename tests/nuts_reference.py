"""A plain reference of one NUTS transition of one chain -- TEST INFRASTRUCTURE ONLY (a helper module, imported by the NUTS tests).

Written from the semantics of DESIGN.md "NUTS" and from nothing else: it shares no arithmetic with the kernel (logreg_amd/csrc/lr_nuts.h),
the CPU test double (tests/host/lr_cpu_twin_nuts.c) or `kernels._numpy_nuts`, which all use the iterative checkpoint scheme.  Here

* the momenta of the subtree's leaves (and of the whole tree) are kept in lists; no checkpoint array, no bit-count indexing;
* after leaf i of a subtree every aligned span `[i + 1 - 2^j, i]` (j >= 1, 2^j divides i + 1) is tested with
  turning(p[first], p[last], sum of p over the span), the sum taken directly from the stored momenta with `math.fsum` per coordinate;
* the tree's and the subtree's momentum sums at a merge are `math.fsum` over their stored leaves as well -- there is no running sum;
* energies and log-weights are combined with `math.fsum`.

Randomness comes through a small stream object (`normals()`, `direction(d)`, `merge_u(d)`, `leaf_u(k)`), called lazily in the order the
text consumes it: `PhiloxStream` is the product's (seed, chain, iteration) stream restated on the oracle's Philox, `NumpyStream` pulls
from NumPy's global generator as `kernels._numpy_nuts` does.

`transition(..., dtype=np.float32)` is the float32 mode: the states, momenta, leapfrog steps, kinetic energies and U-turn dot products
are NumPy float32 in NumPy's own summation order (the model is whatever float32 callables are passed: `F32Model`), the energy
differences, log-weights and draws stay float64 as in the kernel.
"""
from __future__ import annotations

import collections
import math
from dataclasses import dataclass

import numpy as np

TAG_TREE = 0x40000000  # include/logreg_hip_nuts.h LR_NUTS_TAG_TREE | d
TAG_LEAF = 0x20000000  # LR_NUTS_TAG_LEAF | k / 4

DIVERGENCE, SUBTREE, TREE, MERGE2, MERGE3, MERGE23, MAX_DEPTH = "divergence", "subtree", "tree", "merge2", "merge3", "merge2+3", "max_depth"
REASONS = (DIVERGENCE, SUBTREE, TREE, MERGE2, MERGE3, MAX_DEPTH)  # MERGE23 (both across-merge checks, not the whole tree) is counted apart


def u24(w: int) -> float:
    """the 24-bit uniform of a stream word (DESIGN.md "Randomness")"""
    return ((int(w) >> 8) + 0.5) / 2 ** 24


class PhiloxStream:
    """The draws of (seed, chain, iteration) as the product lays them out (DESIGN.md "NUTS", stream tags)."""

    def __init__(self, seed, chain, it, p):
        self.seed, self.chain, self.it, self.p = int(seed), int(chain), int(it), int(p)
        self._key = (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
        self._blocks = {}

    def _block(self, tag):
        if tag not in self._blocks:
            from oracle.oracle import philox4x32_10
            self._blocks[tag] = philox4x32_10((self.chain & 0xFFFFFFFF, self.it & 0xFFFFFFFF, (self.it >> 32) & 0xFFFFFFFF, tag), self._key)
        return self._blocks[tag]

    def normals(self):
        from oracle.oracle import draws
        return np.asarray(draws(self.seed, self.chain, self.it, self.p)[0], dtype=np.float64)

    def direction(self, d):
        return 1 if (self._block(TAG_TREE | d)[0] >> 31) & 1 else -1

    def merge_u(self, d):
        return u24(self._block(TAG_TREE | d)[1])

    def leaf_u(self, k):
        return u24(self._block(TAG_LEAF | (k // 4))[k % 4])


class NumpyStream:
    """NumPy's global generator, pulled lazily: every call draws, so the order of the calls is the order of the text."""

    def __init__(self, p):
        self.p = int(p)

    def normals(self):
        return np.random.randn(self.p)

    def direction(self, d):
        return 1 if np.random.rand() < 0.5 else -1

    def merge_u(self, d):
        return float(np.random.rand())

    def leaf_u(self, k):
        return float(np.random.rand())


class F32Model:
    """The logistic-regression model in NumPy float32, NumPy's own summation order (the float32 mode's model)."""

    def __init__(self, X, y, pscale):
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        self.n, self.p = self.X.shape
        ps = np.broadcast_to(np.asarray(pscale, dtype=np.float64), (self.p,))
        self.inv_var = (1.0 / (ps * ps)).astype(np.float32)
        self.lprior_const = float(np.sum(-0.5 * math.log(2.0 * math.pi) - np.log(ps)))
        self.sign = (2.0 * self.y - 1.0).astype(np.float32)

    def lpost(self, q):
        q = np.asarray(q, dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            t = -self.sign * (self.X @ q)
            ll = -np.sum(np.logaddexp(np.float32(0), t), dtype=np.float32)
            return float(ll) + self.lprior_const - 0.5 * float(np.sum(q * q * self.inv_var, dtype=np.float32))

    def glp(self, q):
        q = np.asarray(q, dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            r = self.y - np.float32(1) / (np.float32(1) + np.exp(-(self.X @ q)))
            return (self.X.T @ r - q * self.inv_var).astype(np.float32)


@dataclass
class Transition:
    x: np.ndarray          # the new state
    depth: int             # signed: negated when the iteration diverged
    n_leaf: int            # leapfrog steps taken
    accept_stat: float     # the iteration's acceptance statistic (mean over its leaves): what accept_stat_sum gains
    divergent: bool
    hit: bool              # max-depth hit
    reason: str
    margin: float          # smallest relative distance of any decision from its threshold
    turn_span: int = 0     # reason == SUBTREE: the shortest span that turned at the stopping leaf
    prop_leaf: int = -1    # the leaf k (in the iteration's order) whose point is the new state; -1: the chain stayed


def _fsum(v):
    """math.fsum; NaN where it refuses (infinities of both signs, an overflowing partial sum)"""
    try:
        return math.fsum(v)
    except (ValueError, OverflowError):
        return math.nan


def _turning(c, a, b, rho, dt):
    """-> (turned, margin).  rho' = rho - (a + b) / 2; (a/dmm) . rho' <= 0 or (b/dmm) . rho' <= 0"""
    r = (rho - dt(0.5) * (a + b)).astype(dt)
    ca, cb = (c * a).astype(dt), (c * b).astype(dt)
    if dt is np.float64:
        sa, sb = _fsum((ca * r).tolist()), _fsum((cb * r).tolist())
    else:
        sa, sb = float(np.dot(ca, r)), float(np.dot(cb, r))
    nr = float(np.linalg.norm(r.astype(np.float64)))
    margin = math.inf
    for s, v in ((sa, ca), (sb, cb)):
        den = float(np.linalg.norm(v.astype(np.float64))) * nr
        margin = min(margin, abs(s) / den if den > 0 and math.isfinite(den) else 0.0)
    return (sa <= 0 or sb <= 0), margin


def _colsum(rows, dt):
    """sum of the stored momenta, coordinate by coordinate, exactly rounded"""
    a = np.asarray(rows, dtype=np.float64)
    return np.array([_fsum(a[:, j].tolist()) for j in range(a.shape[1])]).astype(dt)


def _lae(a, b):
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def transition(lpost, glp, x, eps, dmm, max_depth, stream, dtype=np.float64) -> Transition:
    """One NUTS iteration (DESIGN.md "NUTS", "One iteration" 1-4) from the state x."""
    dt = np.float64 if np.dtype(dtype) == np.float64 else np.float32
    x = np.asarray(x, dtype=dt)
    n = len(x)
    dm = np.broadcast_to(np.asarray(dmm, dtype=np.float64), (n,))
    c = (1.0 / dm).astype(dt)
    step = (float(eps) / dm).astype(dt)
    heps = dt(0.5 * float(eps))

    def kinetic(p):
        t = (p * p * c).astype(dt)
        return _fsum(t.tolist()) if dt is np.float64 else float(np.sum(t, dtype=dt))

    margin = [math.inf]

    def note(m):
        if m < margin[0]:
            margin[0] = m

    with np.errstate(all="ignore"):
        lp = float(lpost(x))
        g = np.asarray(glp(x), dtype=dt)
        p0 = (np.asarray(stream.normals(), dtype=np.float64) * np.sqrt(dm)).astype(dt)
        H0 = _fsum((0.5 * kinetic(p0), -lp))
        # the tree in trajectory order: its leaves' momenta, and (q, p, g) of both ends
        tree_p = [p0]
        ends = {-1: (x, p0, g), 1: (x, p0, g)}
        W, prop, prop_k = 0.0, x, -1
        acc, n_leaf, depth = [], 0, 0
        for d in range(max_depth):
            depth = d + 1
            sgn = stream.direction(d)
            q, p, g = ends[sgn]
            p_inner_old, p_outer_old = p, ends[-sgn][1]
            sub_p, sub_prop, sub_k, Ws = [], None, -1, 0.0
            for i in range(2 ** d):
                k = n_leaf
                p = (p + dt(sgn) * heps * g).astype(dt)
                q = (q + dt(sgn) * step * p).astype(dt)
                lpl, g = float(lpost(q)), np.asarray(glp(q), dtype=dt)
                p = (p + dt(sgn) * heps * g).astype(dt)
                n_leaf += 1
                delta = _fsum((0.5 * kinetic(p), -lpl, -H0))
                if not math.isfinite(delta) or delta > 1000.0:
                    if math.isfinite(delta):
                        note(abs(delta - 1000.0) / 1000.0)
                    acc.append(0.0)
                    return Transition(prop, -depth, n_leaf, math.fsum(acc) / n_leaf, True, False, DIVERGENCE, margin[0], 0, prop_k)
                note(abs(delta - 1000.0) / 1000.0)
                acc.append(1.0 if delta <= 0.0 else math.exp(-delta))
                sub_p.append(p)
                if i == 0:
                    Ws, sub_prop, sub_k = -delta, q, k
                else:
                    Wn = _lae(Ws, -delta)
                    u, prob = stream.leaf_u(k), math.exp(-delta - Wn)
                    note(abs(u - prob))
                    if u < prob:
                        sub_prop, sub_k = q, k
                    Ws = Wn
                # every aligned span that this leaf closes
                turned_spans, length = [], 2
                while (i + 1) % length == 0:
                    first = i + 1 - length
                    t, m = _turning(c, sub_p[first], sub_p[i], _colsum(sub_p[first:i + 1], dt), dt)
                    note(m)
                    if t:
                        turned_spans.append(length)
                    length *= 2
                if turned_spans:
                    return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, False, SUBTREE, margin[0], min(turned_spans), prop_k)
            # the subtree is complete: merge it
            u, prob = stream.merge_u(d), math.exp(min(Ws - W, 700.0))
            note(abs(u - prob))
            if u < prob:
                prop, prop_k = sub_prop, sub_k
            W = _lae(W, Ws)
            rho_old, rho_sub = _colsum(tree_p, dt), _colsum(sub_p, dt)
            tree_p = tree_p + sub_p if sgn > 0 else sub_p[::-1] + tree_p
            ends[sgn] = (q, p, g)
            rho = _colsum(tree_p, dt)
            p_first, p_outer_new = sub_p[0], sub_p[-1]
            t1, m1 = _turning(c, ends[-1][1], ends[1][1], rho, dt)
            t2, m2 = _turning(c, p_outer_old, p_first, (rho_old + p_first).astype(dt), dt)
            t3, m3 = _turning(c, p_outer_new, p_inner_old, (rho_sub + p_inner_old).astype(dt), dt)
            note(min(m1, m2, m3))
            if t1 or t2 or t3:
                reason = TREE if t1 else (MERGE23 if t2 and t3 else (MERGE2 if t2 else MERGE3))
                return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, False, reason, margin[0], 0, prop_k)
        return Transition(prop, depth, n_leaf, math.fsum(acc) / n_leaf, False, True, MAX_DEPTH, margin[0], 0, prop_k)


# ---- teacher-forced comparison of an implementation of the ABI (the kernel, or the CPU test double) with the reference ----------------
def synthetic_model(p, n, seed):
    """-> X [n, p] (intercept first), y, pscale: a small logistic regression whose posterior has unequal scales"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1)) * rng.uniform(0.3, 2.0, p - 1)])
    beta = rng.standard_normal(p) * 0.7
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return X, y, np.full(p, 2.0)


def run_stepwise(la, model, q0, K, eps, dmm, max_depth, seed, chain_offset=0, iter_offset=0, forced=None, **chainset_kw):
    """K iterations at thin 1 through the Python face, one launch per iteration so that every transition has its own counters.
    Iteration k starts from the previous output, or with `forced` (another implementation's steps) from that one's input.
    -> list over k of dict(x_in [C, p], x_out, depth [C] signed, n_leapfrog, divergent, max_depth_hits, accept_stat_sum)."""
    k = la.nutsKernel(model.lpost, model.glp, eps=eps, dmm=dmm, max_depth=max_depth)
    x = np.ascontiguousarray(np.atleast_2d(q0), dtype=model.np_dtype)
    steps = []
    for it in range(K):
        if forced is not None:
            x = forced[it]["x_in"]
        cs = la.ChainSet(k, x, seed=seed, chain_offset=chain_offset, **chainset_kw)
        cs.iter_offset = iter_offset + it
        d = la.DeviceArray(model.device, (1, cs.C), np.int8)
        out = cs.advance(1, 1, depth=d).to_host()[0]
        cn = cs.get_counters()
        steps.append(dict(x_in=x, x_out=out, depth=d.to_host()[0].astype(int), **{f: np.array(cn[f]) for f in
                          ("n_leapfrog", "divergent", "max_depth_hits", "accept_stat_sum")}))
        x = out
    return steps


def reference_steps(lpost, glp, steps, eps, dmm, max_depth, seed, chain_offset=0, iter_offset=0, dtype=np.float64):
    """the reference transition of every (k, chain) of `steps`, each from the implementation's own input state"""
    p = steps[0]["x_in"].shape[1]
    return [[transition(lpost, glp, s["x_in"][c], eps, dmm, max_depth, PhiloxStream(seed, chain_offset + c, iter_offset + k, p), dtype)
             for c in range(s["x_in"].shape[0])] for k, s in enumerate(steps)]


def compare(steps, refs, min_margin):
    """-> (n, skipped, mismatches, worst): transitions compared, skipped for a reference margin below min_margin, descriptions of
    those whose exact fields differ, and the largest relative deviation of a state or acceptance statistic among the others
    (relative to the largest magnitude of the state: a coordinate near zero carries the rounding of the others)."""
    n = skipped = 0
    mism, worst = [], 0.0
    for k, (s, row) in enumerate(zip(steps, refs)):
        for c, r in enumerate(row):
            n += 1
            if not r.margin >= min_margin and not np.isnan(s["x_in"][c]).any():
                skipped += 1
                continue
            got = (int(s["depth"][c]), int(s["n_leapfrog"][c]), int(s["divergent"][c]), int(s["max_depth_hits"][c]))
            want = (r.depth, r.n_leaf, int(r.divergent), int(r.hit))
            if got != want:
                mism.append(f"k={k} chain={c} (depth, leaves, divergent, hit): got {got}, reference {want} [{r.reason}, margin {r.margin:.3g}]")
                continue
            a, b = np.asarray(s["x_out"][c], dtype=np.float64), np.asarray(r.x, dtype=np.float64)
            if np.isnan(b).any():
                if not np.array_equal(a, b, equal_nan=True):
                    mism.append(f"k={k} chain={c}: a non-finite state moved")
                continue
            dev = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
            dev = max(dev, abs(float(s["accept_stat_sum"][c]) - r.accept_stat) / max(r.accept_stat, 1e-300) if r.accept_stat > 0 else 0.0)
            worst = max(worst, dev) if math.isfinite(dev) else math.inf
    return n, skipped, mism, worst


# ---- the cases of the CPU and GPU comparisons ------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "p n eps max_depth unit C K seed chain_offset iter_offset start_scale")

MIN_MARGIN = 1e-9   # a transition may be left out of a float64 comparison only below this reference margin (at most 1 in 1000)
# The bounds below are measurements on the CPU (profiles/r8_nuts_reference.txt); none is taken from the kernel.
F64_TOL = 8.3e-12   # 10 x the largest relative deviation between the CPU double and the reference (8.24e-13 over CPU_CASES)
F32_TAU = 4.0e-6    # float32 kernel: 8 x the largest float64 margin at which the reference's float32 mode disagreed with its float64
                    # mode (4.945e-07: 2 disagreements in 380 160 transitions of F32_CASES, `python tests/nuts_reference.py 48`)
F32_STATE_TOL = 1.64e-3  # ... and 8 x their largest relative deviation where they agreed (2.04e-04, same run)


def case_metric_and_start(case):
    """-> dmm (1.0, or p unequal positive scales), q0 [C, p]"""
    rng = np.random.default_rng(1000 * case.p + case.max_depth)
    dmm = 1.0 if case.unit else rng.uniform(0.3, 3.0, case.p)
    return dmm, case.start_scale * rng.standard_normal((case.C, case.p))


def _cpu_cases():
    cases = []
    widths = (2, 3, 4, 5, 8, 9, 15, 16, 17, 24, 31, 32)
    for i, p in enumerate(widths):
        n = (21, 37, 45, 53)[i % 4]  # never a multiple of 16
        unit = i % 2 == 0
        # shallow trees, many of them: whole-tree and across-merge stops, short subtree U-turns
        cases.append(Case(p, n, (0.5, 0.35, 0.7)[i % 3], 6, unit, 24, 10, 11 + i, 3 + i, 5 + i, 1.0))
        # large steps from the tails: divergences, and trees that end at their first doublings
        cases.append(Case(p, n, (1.6, 2.2)[i % 2], 3, not unit, 16, 6, 40 + i, 1000 + i, 17, 3.0))
        # max_depth 1 and 2: nothing but hits, merges and the first across-merge checks
        cases.append(Case(p, n, 0.2, 1 + i % 2, unit, 8, 4, 70 + i, 7, 2 ** 20 + i, 1.0))
    # deep trees: long spans, the leaf-uniform block boundary at leaf 64, max-depth hits at depth 10
    cases.append(Case(3, 37, 0.01, 10, False, 6, 4, 5, 2, 2 ** 32 + 7, 1.0))   # the high iteration word
    cases.append(Case(9, 21, 0.02, 10, True, 6, 4, 6, 65, 2 ** 33 + 1, 1.0))
    cases.append(Case(17, 45, 0.03, 10, False, 6, 4, 7, 129, 9, 1.0))
    cases.append(Case(32, 53, 0.03, 10, True, 6, 4, 8, 255, 3, 1.0))
    cases.append(Case(8, 37, 0.001, 10, True, 3, 3, 9, 4, 1, 1.0))             # saturated: every tree 1023 leaves
    return cases


CPU_CASES = _cpu_cases()


def _gpu_f64_cases():
    """every width class of the kernel (P = 4, 8, 16 with one coordinate per lane, 32 with two) on both sides of its boundary, chain
    counts that leave partial waves and workgroups, max_depth 10: small steps for deep trees (the second leaf-uniform block at leaf
    64, checkpoints up to index 8), and large steps from the tails (divergences and early stops beside building chains)"""
    deep = {3: (257, 2, 0.02), 4: (65, 3, 0.03), 5: (3, 8, 0.02), 8: (1, 10, 0.02), 9: (65, 3, 0.02), 16: (257, 2, 0.03),
            17: (3, 8, 0.02), 31: (1, 10, 0.02), 32: (65, 3, 0.03)}
    cases = []
    for i, (p, (C, K, eps)) in enumerate(deep.items()):
        n = (21, 37, 45, 53)[i % 4]
        cases.append(Case(p, n, eps, 10, i % 2 == 1, C, K, 300 + i, 11 * i, 2 ** 32 * (i % 2) + i, 1.0))
        cases.append(Case(p, n, (1.6, 0.6, 2.2)[i % 3], 10, i % 2 == 0, (65, 3, 257, 1)[i % 4], 3, 400 + i, 5 + i, 1 + i, 3.0))
    return cases


GPU_F64_CASES = _gpu_f64_cases()
# float32: all four width classes, moderate trees (every leaf adds decisions that float32 rounding can move) and a few hundred rows
# (the rounding of the log-likelihood sum grows with its size)
F32_CASES = [Case(p, n, eps, 10, i % 2 == 0, 129, 4, 500 + i, 7 * i, 3 + i, 1.0)
             for i, (p, n, eps) in enumerate(((3, 203, 0.15), (8, 157, 0.12), (9, 301, 0.1), (16, 119, 0.1), (17, 251, 0.08), (32, 185, 0.08)))]


def float32_problem(case):
    """-> X, y, pscale with X rounded to float32 (as float64 values), dmm, q0 rounded to float32"""
    X, y, ps = synthetic_model(case.p, case.n, 100 + case.p)
    dmm, q0 = case_metric_and_start(case)
    return X.astype(np.float32).astype(np.float64), y, ps, dmm, q0.astype(np.float32)


def shape_of(t):
    return (t.depth, t.n_leaf, bool(t.divergent), bool(t.hit))


def measure_float32_mode(cases=None):
    """The reference's float32 mode against its float64 mode, teacher-forced along the float32 mode's chain.  -> dict: n, disagree
    (tree shape, flags or selected leaf differ), tau (the largest float64 margin among those), dev (the largest relative deviation
    of state or acceptance statistic among the others), margins (every float64 margin), share (of margins below F32_TAU)."""
    from oracle.oracle import OracleModel
    tau = dev = 0.0
    margins, disagree = [], 0
    for case in cases or F32_CASES:
        X, y, ps, dmm, q0 = float32_problem(case)
        m32, m64 = F32Model(X, y, ps), OracleModel(X, y, ps)
        x = q0
        for k in range(case.K):
            nxt = []
            for c in range(case.C):
                args = (case.eps, dmm, case.max_depth, PhiloxStream(case.seed, case.chain_offset + c, case.iter_offset + k, case.p))
                t32 = transition(m32.lpost, m32.glp, x[c], *args, dtype=np.float32)
                t64 = transition(m64.lpost, m64.glp, x[c].astype(np.float64), *args)
                nxt.append(t32.x)
                margins.append(t64.margin)
                if shape_of(t32) != shape_of(t64) or t32.prop_leaf != t64.prop_leaf:
                    disagree += 1
                    tau = max(tau, t64.margin)
                else:
                    a, b = t32.x.astype(np.float64), t64.x
                    dev = max(dev, float(np.max(np.abs(a - b)) / np.max(np.abs(b))), abs(t32.accept_stat - t64.accept_stat) / t64.accept_stat)
            x = np.array(nxt, dtype=np.float32)
    margins = np.array(margins)
    return dict(n=len(margins), disagree=disagree, tau=tau, dev=dev, margins=margins, share=float(np.mean(margins < F32_TAU)))


def _measure_one(case):
    m = measure_float32_mode([case])
    return case, m


if __name__ == "__main__":
    # python tests/nuts_reference.py [replicates]: the float32 measurement behind F32_TAU / F32_STATE_TOL on the float32 cases, each
    # widened to 330 chains and repeated under `replicates` seeds (default 24: 190 080 transitions, 61 x the test's), in 16 processes
    import multiprocessing
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    with multiprocessing.Pool(16) as pool:
        res = pool.map(_measure_one, [c._replace(C=330, seed=c.seed + 1000 * r) for r in range(reps) for c in F32_CASES], chunksize=1)
    tau = max(m["tau"] for _, m in res)
    dev = max(m["dev"] for _, m in res)
    mg = np.concatenate([m["margins"] for _, m in res])
    for p_ in sorted({c.p for c, _ in res}):
        sel = [m for c, m in res if c.p == p_]
        print(f"p={p_}: {sum(m['n'] for m in sel)} transitions, {sum(m['disagree'] for m in sel)} disagree, largest disagreeing margin "
              f"{max(m['tau'] for m in sel):.4g}, largest relative deviation {max(m['dev'] for m in sel):.4g}")
    print("smallest margins:", np.sort(mg)[:5])
    print(f"all: {len(mg)} transitions, {sum(m['disagree'] for _, m in res)} disagree; largest disagreeing margin {tau:.4g} (x 8 = {8 * tau:.4g}); "
          f"largest relative deviation {dev:.4g} (x 8 = {8 * dev:.4g}); share of margins below 8 x tau {np.mean(mg < 8 * tau):.5f}, "
          f"below F32_TAU = {F32_TAU:g}: {np.mean(mg < F32_TAU):.5f}")
