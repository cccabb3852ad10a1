"""The Polya-Gamma Gibbs sampler (include/logreg_hip_pg.h) -- everything that can be checked without a GPU: the reference draw's moments
against the closed forms, the CPU test double (tests/host/lr_cpu_twin_pg.c) against the independent NumPy reference
(tests/pg_reference.py) sweep by sweep and omega by omega, the tolerances of tests/test_gpu_pg.py re-measured, the Python face
(pgKernel, ChainSet, mcmc, mcmc_sharded's slicing) on the double, the ABI tables and exports of both builds, and the host side of the
run under AddressSanitizer and UBSan as a stand-alone program (tests/host/pg_harness.cpp)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import host_build
import pg_reference as pr
import twin_pg

WANT = ["lr_pg_omega", "lr_run_pg"]
N_DRAWS = 400_000
C64 = [0, 1e-8, 0.1, 1, 3.12, 3.13, 10, 40, 100, 1000]
C32 = [0, 1e-8, 0.1, 1, 3.12, 3.13, 10, 40, 80]


@pytest.fixture(scope="module", autouse=True)
def _pg_twin():
    twin_pg.install()
    yield
    twin_pg.uninstall()


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def _moments(c):
    """E omega = tanh(c/2) / (2c), Var omega = (sinh c - c) / (4 c^3 cosh^2(c/2)); limits 1/4 and 1/24 at c -> 0.  Past c = 30 the ratio
    sinh c / cosh^2(c/2) is 2 to the last bit and (sinh c - c) / cosh^2(c/2) = 2 - c / cosh^2(c/2) avoids the overflow."""
    if c < 1e-4:
        return 0.25, 1.0 / 24.0
    mean = np.tanh(c / 2) / (2 * c)
    if c > 30:
        return mean, (2.0 - (c / np.cosh(c / 2)) / np.cosh(c / 2) if c < 1400 else 2.0) / (4 * c ** 3)
    return mean, (np.sinh(c) - c) / (4 * c ** 3 * np.cosh(c / 2) ** 2)


@pytest.mark.parametrize("dtype,cs", [(np.float64, C64), (np.float32, C32)], ids=["float64", "float32"])
def test_reference_draw_has_the_moments_of_pg(dtype, cs):
    """4e5 draws per c: z of the mean from the closed-form variance, z of the variance from the sample fourth moment; |z| < 4.2."""
    for k, c in enumerate(cs):
        i = np.arange(N_DRAWS)
        d = pr.draw(np.full(N_DRAWS, c), 2021, i // 1000 + 7, 3 + k, i % 1000, dtype)
        w = d["omega"].astype(np.float64)
        assert np.all(np.isfinite(w)) and np.all(w > 0)
        mean, var = _moments(c)
        zm = (w.mean() - mean) / np.sqrt(var / N_DRAWS)
        s2 = w.var()
        m4 = np.mean((w - w.mean()) ** 4)
        zv = (s2 - var) / np.sqrt((m4 - s2 * s2) / N_DRAWS)
        print(f"{np.dtype(dtype).name} c = {c:g}: z(mean) {zm:+.2f}, z(var) {zv:+.2f}, var ratio {s2 / var:.4f}, proposals per draw {d['proposals'].mean():.5f}, "
              f"series terms per draw {d['terms'].mean():.4f}")
        assert abs(zm) < 4.2 and abs(zv) < 4.2, (c, zm, zv)
        assert d["proposals"].mean() < 1.0015  # theory: <= 1.0009


def _double_sweep(la, case, dtype="float64"):
    """one sweep of the case on the double, through the C ABI: -> (omega [C, n], new states [C, p], counters [C])"""
    from logreg_amd import _lib
    L = _lib.load_pg()
    X, y, ps, st = pr.make_case(case)
    m = la.LogReg(X, y, ps, dtype=dtype)
    st = np.ascontiguousarray(st, dtype=m.np_dtype)
    opts = _lib.RunOpts(n_chains=case.C, chain_offset=case.chain_offset, thin=1, iters=1, iter_offset=case.iter_offset, seed=case.seed, group=0,
                        mode=_lib.MODE_AUTO, on_device=0)
    om = np.empty((case.C, case.n), dtype=m.np_dtype)
    before = st.copy()
    assert L.lr_pg_omega(m.handle, st.ctypes.data, ctypes.byref(opts), om.ctypes.data) == 0, L.lr_last_error()
    assert np.array_equal(st, before)  # the state is not moved
    cn = np.zeros(case.C, dtype=la.kernels.PG_COUNTERS)
    assert L.lr_run_pg(m.handle, st.ctypes.data, ctypes.byref(opts), None, cn.ctypes.data) == 0, L.lr_last_error()
    m.close()
    return om, st, cn


def test_the_double_equals_the_reference_and_fixes_the_float64_tolerance(la):
    """Sweep by sweep and omega by omega over pr.CPU_CASES (every width 3 .. 32, n = 1 .. 257, 1 .. 257 chains, nonzero offsets): the
    counters -- the number of rounds and of series terms of every chain -- are EQUAL, so every decision was; the largest relative
    deviation of omega and of the state, times 10, is pr.F64_TOL."""
    worst_om = worst_st = 0.0
    for case in pr.CPU_CASES:
        X, y, ps, st = pr.make_case(case)
        ref = pr.sweep(pr.signed_rows(X, y), ps, st, case.seed, np.arange(case.C) + case.chain_offset, case.iter_offset)
        om, new, cn = _double_sweep(la, case)
        assert np.array_equal(cn["proposals"], ref.proposals) and np.array_equal(cn["series_terms"], ref.terms), case
        assert not ref.skipped.any() and not cn["skipped"].any()
        assert np.all(ref.proposals >= case.n)
        worst_om, worst_st = max(worst_om, pr.omega_dev(om, ref.omega)), max(worst_st, pr.rel_dev(new, ref.beta))
    worst = max(worst_om, worst_st)
    print(f"double vs reference, float64: largest relative deviation of omega {worst_om:.4g}, of the state {worst_st:.4g}; F64_TOL = {pr.F64_TOL:g}")
    assert {c.p for c in pr.CPU_CASES} == {3, 4, 5, 8, 9, 16, 17, 31, 32} and {c.n for c in pr.CPU_CASES} == {1, 15, 17, 200, 257}
    assert {c.C for c in pr.CPU_CASES} == {1, 3, 65, 257} and all(c.chain_offset > 0 and c.iter_offset > 0 for c in pr.CPU_CASES)
    assert {c.p for c in pr.GPU_CASES} == {3, 4, 5, 8, 9, 16, 17, 31, 32} and {c.n for c in pr.GPU_CASES} == {15, 17, 200} and {c.C for c in pr.GPU_CASES} == {1, 3, 65, 257}
    assert 10 * worst <= pr.F64_TOL <= 100 * worst  # the constant is the measurement, neither smaller nor padded


def _f32_pair(cases, reps):
    """the reference's float32 mode against its float64 mode on float32-rounded data"""
    tau = dev = sdev = 0.0
    margins, chains, whole = [], 0, 0
    for case in cases:
        X, y, ps, st = pr.make_case(case)
        X32, st32 = X.astype(np.float32).astype(np.float64), st.astype(np.float32).astype(np.float64)
        Xs = pr.signed_rows(X32, y)
        ch = np.arange(case.C) + case.chain_offset
        for rep in range(reps):
            a = pr.sweep(Xs, ps, st32, case.seed, ch, case.iter_offset + rep, np.float64)
            b = pr.sweep(Xs, ps, st32, case.seed, ch, case.iter_offset + rep, np.float32)
            rel = np.abs(b.omega.astype(np.float64) - a.omega) / a.omega
            dis = rel > 1e-3  # another decision gives another draw, not a rounding error
            if dis.any():
                tau = max(tau, float(a.margin[dis].max()))
            dev = max(dev, float(rel[~dis].max()))
            margins.append(a.margin)
            ok = ~dis.any(axis=1)
            sdev = max(sdev, pr.rel_dev(b.beta[ok], a.beta[ok]))
            chains += case.C
            whole += int(np.sum(np.all(a.margin >= pr.F32_TAU, axis=1)))
    return tau, dev, sdev, np.concatenate([m.ravel() for m in margins]), chains, whole


def test_float32_mode_of_the_reference_fixes_the_float32_pair():
    """pr.F32_TAU is 8 x the largest float64 margin at which the two modes drew differently, pr.F32_OMEGA_TOL and pr.F32_STATE_TOL 8 x their
    largest relative deviation where they agreed, all from the larger run recorded in profiles/r21_pg.txt; this run must not exceed
    them.  At most 1 % of the draws fall below the threshold, and at most 10 % of the chains of pr.F32_CASES hold such a draw."""
    tau, dev, sdev, margins, _, _ = _f32_pair(pr.GPU_CASES, 4)
    share = float(np.mean(margins < pr.F32_TAU))
    print(f"float32 vs float64 mode, omega shapes: {margins.size} draws, largest disagreeing margin {tau:.4g}, largest omega deviation {dev:.4g}; "
          f"F32_TAU = {pr.F32_TAU:g}, F32_OMEGA_TOL = {pr.F32_OMEGA_TOL:g}, share below the threshold {share:.2e}")
    assert 8 * tau <= pr.F32_TAU and 8 * dev <= pr.F32_OMEGA_TOL and share <= 0.01
    tau, dev, sdev, margins, chains, whole = _f32_pair(pr.F32_CASES, 4)
    print(f"float32 vs float64 mode, transition shapes: {chains} chains, {chains - whole} with a draw below the threshold, largest state deviation {sdev:.4g}; "
          f"F32_STATE_TOL = {pr.F32_STATE_TOL:g}")
    assert 8 * tau <= pr.F32_TAU and 8 * dev <= pr.F32_OMEGA_TOL and 8 * sdev <= pr.F32_STATE_TOL
    assert all(c.n <= 40 for c in pr.F32_CASES) and chains - whole <= 0.10 * chains


def test_python_face_on_the_double(la, pima, pscale, map_beta, tmp_path):
    X, y = pima
    with pytest.raises(TypeError, match="X, y"):
        la.pgKernel(lambda b: -0.5 * np.sum(b * b))
    for dtype in ("float64", "float32"):
        m = la.LogReg(X, y, pscale, dtype=dtype)
        with pytest.raises(TypeError, match="not from a log-density"):
            la.pgKernel(m.glp)
        k = la.pgKernel(m.lpost)
        assert isinstance(k, la.FusedKernel) and k.kind == "pg" and k.params == {} and k.model is m
        rng = np.random.default_rng(3)
        q0 = map_beta + 0.05 * rng.standard_normal((9, 8))
        full, info = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, return_info=True)
        assert full.shape == (6, 9, 8) and full.dtype == m.np_dtype
        # the reference run (float64 model: every bit of the arithmetic is restated independently)
        if dtype == "float64":
            ref, prop, term, skip = pr.run(pr.signed_rows(X, y), pscale, q0, 17, 2, 0, 6, 2)
            assert pr.rel_dev(full, ref) <= pr.F64_TOL * 12  # (12 sweeps compound)
            assert np.array_equal(info["proposals"], prop) and np.array_equal(info["series_terms"], term) and not skip.any()
        n, sweeps = m.n, 12
        assert np.all(info["proposals"] >= n * sweeps) and np.all(info["proposals"] < 1.01 * n * sweeps) and info["skipped"].sum() == 0
        assert np.allclose(info["proposals_per_draw"], info["proposals"] / (n * sweeps)) and info["iterations"] == sweeps
        assert info["plan"]["group"] >= 1
        assert np.array_equal(la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, chunk=4), full)  # chunks equal the whole
        sh, shi = la.mcmc(q0[3:8], k, thin=2, iters=6, verb=False, seed=17, chain_offset=5, plan_chains=9, plan_first=2, return_info=True)
        assert np.array_equal(sh, full[:, 3:8]) and np.array_equal(shi["proposals"], info["proposals"][3:8])  # a shard equals its slice
        single = la.mcmc(map_beta, k, thin=1, iters=3, verb=False, seed=5)
        assert single.shape == (3, 8) and single.dtype == np.float64
        x1 = k(map_beta)  # one step, the reference's per-step signature
        assert x1.shape == (8,) and np.all(np.isfinite(x1)) and not np.array_equal(x1, map_beta)
        # checkpoint: the counters travel
        cs = la.ChainSet(k, q0, seed=17, chain_offset=2)
        a = cs.advance(2, 2).to_host()
        cs2 = la.ChainSet.resume(k, cs.save(tmp_path / f"pg_{dtype}"))
        b = cs2.advance(4, 2).to_host()
        assert np.array_equal(np.concatenate([a, b]), full)
        for f in ("proposals", "series_terms", "skipped"):
            assert np.array_equal(cs2.get_counters()[f], info[f]), f
        with pytest.raises(ValueError, match="Polya-Gamma"):
            la.ChainSet(la.hmcKernel(m.lpost, m.glp, 0.01, 5, 1.0), q0, seed=1).pg_info()
        # a non-finite start stays in place and is counted
        bad = q0.copy()
        bad[1, 3], bad[4, 0], bad[6, 7] = np.nan, np.inf, -np.inf
        out, binfo = la.mcmc(bad, k, thin=2, iters=3, verb=False, seed=17, return_info=True)
        for c in (1, 4, 6):
            assert binfo["skipped"][c] == 6 and binfo["proposals"][c] == 0 and binfo["series_terms"][c] == 0
            assert np.array_equal(out[:, c], np.broadcast_to(bad[c].astype(m.np_dtype), (3, 8)), equal_nan=True)
        good = [c for c in range(9) if c not in (1, 4, 6)]
        assert binfo["skipped"][good].sum() == 0 and np.all(np.isfinite(out[:, good]))
        # summary_only: the streaming statistics of the same run (the accumulators need the device: tests/test_gpu_pg.py)
        res = la.mcmc(q0, k, thin=2, iters=6, verb=False, seed=17, chain_offset=2, summary_only=True)
        assert res["accept_rate"] == 1.0 and res["skipped"].sum() == 0 and np.array_equal(res["proposals"], info["proposals"])
        np.testing.assert_allclose(res["mean"], full.astype(np.float64).mean(axis=(0, 1)), rtol=1e-6)
        m.close()


def test_symbol_tables_match_the_header_and_both_libraries():
    from logreg_amd import _lib, build
    assert _declared("logreg_hip_pg.h") == WANT == sorted(_lib.PG_SYMBOLS)
    assert _declared("logreg_hip.h") == sorted(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 38
    for other in (_lib.SYMBOLS, _lib.NUTS_SYMBOLS, _lib.PREDICT_SYMBOLS, _lib.ACF_SYMBOLS, _lib.MARG_SYMBOLS, _lib.LOO_SYMBOLS, _lib.COV_SYMBOLS, _lib.ADAPT_SYMBOLS,
                  _lib.DENSE_SYMBOLS):
        assert not set(WANT) & set(other)
    L = ctypes.CDLL(twin_pg.build())
    for s in WANT + _declared("logreg_hip.h"):
        assert hasattr(L, s)
    assert _lib.KIND_BY_NAME["pg"] == 6 and _lib.PG_TAG == 0x10000000 and ctypes.sizeof(_lib.PgCounters) == 24
    import logreg_amd.kernels as K
    assert K.PG_COUNTERS.itemsize == 24 and K.PG_COUNTERS.names == tuple(f for f, _ in _lib.PgCounters._fields_)
    txt = open(os.path.join(REPO, "include", "logreg_hip_pg.h")).read()
    for word in ("#define LR_KIND_PG 6", "#define LR_PG_TAG 0x10000000u", "fit-rjags.R", "precision is IGNORED"):
        assert word in txt, word
    src = build._sources()
    for f in (os.path.join(build.INCLUDE, "logreg_hip_pg.h"), os.path.join(build.CSRC, "lr_pg.h")):
        assert f in src, f
    build.build(verbose=False)
    build.build(verbose=False, alt=True)
    for path in (_lib.LIB_PATH, build.ALT_LIB):
        L = ctypes.CDLL(path)
        for s in WANT:
            assert hasattr(L, s), (path, s)
        exported = os.popen(f"nm -D --defined-only {path}").read()
        assert sorted(set(re.findall(r"\b(lr_run_pg|lr_pg_\w+)\b", exported))) == WANT, path


def test_the_eight_kernels_pass_the_gates_in_both_builds():
    from logreg_amd import build as b, isa_gate
    for alt in (False, True):
        b.build(verbose=False, alt=alt)
        rows = [r for r in b.kernel_resources(alt=alt) if "k_pg<" in r["name"]]
        assert len(rows) == 8 and len(b.unit_objects(alt)) == 13
        for dt in ("float", "double"):
            for P in (4, 8, 16, 32):
                mine = [r for r in rows if f"k_pg<{dt}, {P}>" in r["name"]]
                assert len(mine) == 1 and mine[0]["unit"] == f"lr_inst_{'f32' if dt == 'float' else 'f64'}_p{P}", (alt, dt, P)
        assert all(r["scratch"] == 0 and r["lds"] == 0 and r["vgprs"] + r["agprs"] <= 512 for r in rows), [(r["name"], r["scratch"], r["vgprs"], r["agprs"]) for r in rows]
        assert isa_gate.scan_paths(b.unit_objects(alt)) == []
    b.resource_gate(strict=True, verbose=False)
    b.exec_prologue_gate(strict=True, verbose=False)


def test_host_side_under_asan_and_ubsan():
    """tests/host/pg_harness.cpp, a program of its own, linked with tests/host/hip_stub.cpp, lr_api.hip and the library's instantiation
    objects by tests/host_build.py: the refusals, plan_pg and its reasons, the vector b, and
    runs from host and device memory on the stub."""
    last = host_build.last_line(host_build.run(host_build.harness("pg_harness.cpp")))
    assert last.startswith("pg harness:"), last
