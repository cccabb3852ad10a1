"""NUTS above the kernel, in the GPU-less container: the ABI's symbol tables, the CPU test double of include/logreg_hip_nuts.h
(tests/host/lr_cpu_twin_nuts.c, injected by tests/twin_nuts.py for this module) against the reference's posterior, the Python face
(nutsKernel, ChainSet, mcmc) on it, the generic NumPy NUTS, and the stream layout against the oracle's Philox.
The tree logic itself -- the double and the generic NumPy NUTS, transition by transition against an independent reference at every
width, depth and stop reason -- is tests/test_nuts_reference_cpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

import twin_nuts

PRE = np.array([10.0, 1, 1, 1, 1, 1, 5, 1])  # fit-blackjax-nuts.py:101 `pre`; dmm = 1 / pre


@pytest.fixture(scope="module", autouse=True)
def _nuts_twin():
    twin_nuts.install()
    yield
    twin_nuts.uninstall()


@pytest.fixture(scope="module")
def la():
    import logreg_amd
    return logreg_amd


@pytest.fixture(scope="module")
def models(la, pima, pscale):
    X, y = pima
    return {d: la.LogReg(X, y, pscale, dtype=d) for d in ("float32", "float64")}


def header_symbols(name):
    txt = open(os.path.join(REPO, "include", name)).read()
    return sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", txt)))


def test_symbol_tables_match_the_headers():
    from logreg_amd import _lib
    nuts = header_symbols("logreg_hip_nuts.h")
    assert nuts == ["lr_run_nuts"] and sorted(_lib.NUTS_SYMBOLS) == nuts
    assert sorted(_lib.SYMBOLS) == header_symbols("logreg_hip.h") and not set(nuts) & set(_lib.SYMBOLS)
    L = ctypes.CDLL(twin_nuts.build())
    for s in nuts + header_symbols("logreg_hip.h"):
        assert hasattr(L, s)
    txt = open(os.path.join(REPO, "include", "logreg_hip_nuts.h")).read()
    assert "fit-blackjax-nuts.py:101" in txt and "fit-numpyro.py:36-46" in txt
    from logreg_amd import build
    assert os.path.join(build.INCLUDE, "logreg_hip_nuts.h") in build._sources()  # part of the build id


def test_library_exports_the_nuts_entry_point():
    """The built library (cross-compiled here) exports what logreg_hip_nuts.h declares."""
    import shutil
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc to build the library")
    from logreg_amd import _lib, build
    build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in header_symbols("logreg_hip_nuts.h"):
        assert hasattr(L, s)


def z_scores(summ, ref):
    zm = (summ["mean"] - np.array(ref["mean"])) / np.sqrt(summ["mcse"] ** 2 + np.array(ref["mcse"]) ** 2)
    se_sd = summ["sd"] / np.sqrt(2 * summ["ess"])
    zs = (summ["sd"] - np.array(ref["sd"])) / np.sqrt(se_sd ** 2 + np.array(ref["se_sd"]) ** 2)
    return zm, zs


def test_twin_posterior_matches_the_reference(la, models, map_beta):
    """64 chains, dmm = 1 / pre.  (With this metric Pima's fastest coordinates cap the stable step near 0.003 -- 0.0035 diverges in
    most trees -- and eps = 0.002 builds trees of mean depth 7 to 8; no stable step gives the shallower trees of a better metric.)"""
    ref = load_golden("posterior_hmc.json")["pooled"]
    k = la.nutsKernel(models["float64"].lpost, models["float64"].glp, eps=0.002, dmm=1 / PRE)
    cs = la.ChainSet(k, np.tile(map_beta, (64, 1)), seed=11)
    cs.advance(1, 40, keep=False)
    samples = cs.advance(160, 1).to_host()
    info = cs.nuts_info()
    zm, zs = z_scores(la.summarise(samples, max_chains=64), ref)
    print("z(mean)", np.round(zm, 2), "z(sd)", np.round(zs, 2), "depth", info["mean_depth"].mean())
    assert 5.0 < info["mean_depth"].mean() < 9.5 and info["divergent"].sum() == 0
    assert np.max(np.abs(zm)) < 4.2 and np.max(np.abs(zs)) < 4.2


def test_python_face_shapes_chunks_shards_checkpoint(la, models, map_beta, tmp_path):
    m = models["float32"]
    k = la.nutsKernel(m.lpost, m.glp, eps=0.002, dmm=1 / PRE, max_depth=6)
    assert isinstance(k, la.FusedKernel) and k.kind == "nuts" and k.params["max_depth"] == 6
    q0 = map_beta + 0.01 * np.random.default_rng(1).standard_normal((12, 8))
    full = la.mcmc(q0, k, thin=2, iters=9, verb=False, seed=5)
    assert full.shape == (9, 12, 8) and full.dtype == np.float32
    single = la.mcmc(map_beta, k, thin=2, iters=4, verb=False, seed=5)
    assert single.shape == (4, 8) and single.dtype == np.float64
    assert np.array_equal(la.mcmc(q0, k, thin=2, iters=9, verb=False, seed=5, chunk=2), full)  # chunked
    sh = la.mcmc(q0[4:9], k, thin=2, iters=9, verb=False, seed=5, chain_offset=4, plan_chains=12, plan_first=0)
    assert np.array_equal(sh, full[:, 4:9])  # a shard
    cs = la.ChainSet(k, q0, seed=5)
    a = cs.advance(4, 2).to_host()
    path = cs.save(tmp_path / "nuts")
    cs2 = la.ChainSet.resume(k, path)
    b = cs2.advance(5, 2).to_host()
    assert np.array_equal(np.concatenate([a, b]), full)
    whole = _counters_of(la, k, q0, 9)  # the counters travel with the checkpoint
    for f in ("n_leapfrog", "depth_sum", "divergent", "max_depth_hits"):
        assert np.array_equal(cs2.get_counters()[f], whole[f]), f
    k_other = la.nutsKernel(m.lpost, m.glp, eps=0.002, dmm=1 / PRE, max_depth=7)
    with pytest.raises(ValueError, match="param_max_depth"):
        la.ChainSet.resume(k_other, path)


def _counters_of(la, k, q0, iters):
    cs = la.ChainSet(k, q0, seed=5)
    cs.advance(iters, 2, keep=False)
    return cs.get_counters()


def test_return_info_and_summary_only(la, models, map_beta):
    m = models["float64"]
    k = la.nutsKernel(m.lpost, m.glp, eps=0.002, dmm=1 / PRE, max_depth=5)
    q0 = np.tile(map_beta, (8, 1))
    out, info = la.mcmc(q0, k, thin=1, iters=10, verb=False, seed=3, return_info=True)
    for f in ("n_leapfrog", "divergent", "max_depth_hits", "mean_depth", "mean_accept_stat"):
        assert info[f].shape == (8,), f
    assert np.all(info["n_leapfrog"] <= 10 * 31) and np.all(info["mean_depth"] <= 5) and np.all(info["mean_depth"] >= 1)
    assert np.all((info["mean_accept_stat"] > 0) & (info["mean_accept_stat"] <= 1))
    assert info["plan"]["mode"] in ("lds", "global") and "accepts" not in info
    s = la.mcmc(q0, k, thin=1, iters=10, verb=False, seed=3, summary_only=True)
    np.testing.assert_allclose(s["mean"], out.reshape(-1, 8).mean(axis=0), rtol=1e-12)
    assert 0 < s["accept_rate"] <= 1 and s["n_leapfrog"].sum() == info["n_leapfrog"].sum()


def test_readable_errors(la, pima):
    rng = np.random.default_rng(0)
    wide = la.LogReg(rng.standard_normal((50, 40)), (rng.random(50) < 0.5).astype(float), 1.0)
    with pytest.raises(la.LogregHipError, match="p = 40 > 32"):
        la.mcmc(np.zeros(40), la.nutsKernel(wide.lpost, wide.glp), iters=1, verb=False)
    with pytest.raises(ValueError, match="max_depth"):
        la.nutsKernel(wide.lpost, wide.glp, max_depth=11)


def test_tall_shapes_are_refused_with_the_reason(la):
    """The twin plans one variant whatever the shape; the product's planner refuses rows beyond the LDS with the reason
    (lr_plan.h plan_nuts), checked here in its source and on the GPU by tests/test_gpu_nuts.py."""
    src = open(os.path.join(REPO, "logreg_amd", "csrc", "lr_plan.h")).read()
    body = src[src.index("int plan_nuts("):]
    body = body[:body.index("\n}\n")]
    for reason in ("p = %d > 32", "stepwise (tall-data) engine has no NUTS kernel", "beyond the %zu a"):
        assert reason in body


def test_generic_numpy_nuts_on_a_correlated_gaussian(la):
    cov = np.array([[1.0, 0.8], [0.8, 1.0]])
    prec = np.linalg.inv(cov)
    k = la.nutsKernel(lambda q: -0.5 * q @ prec @ q, lambda q: -prec @ q, eps=0.3, dmm=1.0, max_depth=6)
    assert not isinstance(k, la.FusedKernel)
    np.random.seed(42)
    s = la.mcmc(np.zeros(2), k, thin=1, iters=3000, verb=False)
    assert s.shape == (3000, 2)
    s = s[200:]
    se = 1.0 / np.sqrt(len(s) / 3)  # NUTS draws here are nearly independent; a conservative ESS of a third
    assert np.all(np.abs(s.mean(axis=0)) < 4 * se)
    np.testing.assert_allclose(np.cov(s.T), cov, atol=0.12)


def test_stream_layout_against_the_oracle_philox(la, models, map_beta, oracle_model):
    """max_depth = 1 is one doubling of one leaf: its direction is bit 31 of word x of block 0x40000000 | 0, and the leaf replaces the
    state iff the merge uniform, word y of that block, is below exp(H0 - H1).  Predicted here from oracle.philox4x32_10, the oracle's
    normals and its float64 model, for many (chain, iteration) counters: both outcomes and both directions occur.  A leaf uniform is
    the documented word of its block (tags as the header documents them)."""
    from oracle.oracle import draws, philox4x32_10
    m = models["float64"]
    eps, seed = 0.002, 0x1234_5678_9ABC
    key = (seed & 0xFFFFFFFF, seed >> 32)
    k = la.nutsKernel(m.lpost, m.glp, eps=eps, dmm=1 / PRE, max_depth=1)
    C = 24
    x0 = map_beta + 0.3 * np.array([1.73, 0.065, 0.0068, 0.018, 0.023, 0.043, 0.55, 0.022]) * np.random.default_rng(2).standard_normal((C, 8))
    cs = la.ChainSet(k, x0, seed=seed, chain_offset=5)
    cs.iter_offset = 3
    got = cs.advance(1, 1).to_host()[0]
    seen = set()
    for c in range(C):
        w = philox4x32_10((5 + c, 3, 0, 0x40000000 | 0), key)
        fwd = (int(w[0]) >> 31) == 1
        u = ((int(w[1]) >> 8) + 0.5) / 2 ** 24
        z, _ = draws(seed, 5 + c, 3, 8)
        p = np.asarray(z) * np.sqrt(1 / PRE)
        q, g = x0[c], oracle_model.glp(x0[c])
        h = (1.0 if fwd else -1.0) * 0.5 * eps
        p1 = p + h * g
        q1 = q + (1.0 if fwd else -1.0) * (eps * PRE) * p1
        p1 = p1 + h * oracle_model.glp(q1)
        H0 = 0.5 * np.sum(PRE * p * p) - oracle_model.lpost(q)
        H1 = 0.5 * np.sum(PRE * p1 * p1) - oracle_model.lpost(q1)
        moved = u < np.exp(H0 - H1)
        np.testing.assert_allclose(got[c], q1 if moved else q, rtol=1e-12, atol=1e-14)
        seen.add((fwd, bool(moved)))
    assert len(seen) >= 3, seen
    L = ctypes.CDLL(twin_nuts.build())
    out = (ctypes.c_uint32 * 4)()
    for blk in (0x40000000 | 7, 0x20000000 | 9):
        L.orc_philox4x32_10((ctypes.c_uint32 * 4)(5, 3, 0, blk), (ctypes.c_uint32 * 2)(*key), out)
        assert list(out) == [int(v) for v in philox4x32_10((5, 3, 0, blk), key)]
    txt = open(os.path.join(REPO, "include", "logreg_hip_nuts.h")).read()
    assert "LR_NUTS_TAG_TREE 0x40000000u" in txt and "LR_NUTS_TAG_LEAF 0x20000000u" in txt
