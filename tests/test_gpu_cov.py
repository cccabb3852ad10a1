"""The covariance accumulator on the GPU (include/logreg_hip_cov.h, csrc/lr_cov.h) against tests/cov_reference.py.

For every case of tests/cov_cases.py (both dtypes) and every feeding (one call, chunks of 1, of 7, uneven; host and device memory): the
four tables -- moment, chain_outer, sum, chain_sums -- lie within the forward-error bounds the reference derives from the input alone
(nothing here is measured on the kernel), every entry is finite exactly where the reference's is, moment and chain_outer are symmetric
to the bit, and the bytes of all four are identical across all feedings, a repeat after reset() and the second build of the library.
`python tests/test_gpu_cov.py --measure` prints the error / bound ratios (profiles/r16_cov.txt).
"""
import faulthandler
import sys

import numpy as np
import pytest

import cov_cases as cases
import cov_reference as cr

pytestmark = pytest.mark.gpu
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = cases.case(name, dtype)
        _REF[(name, dtype)] = cr.tables(c["x"], c["center"], c["scale"])
    return _REF[(name, dtype)]


@pytest.fixture(autouse=True)
def step_timeout():
    """Every test under its own time limit: one that hangs ends the whole run (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def la():
    import logreg_amd as la
    return la


def new(la, c):
    return la.Covariance(c["C"], c["p"], c["dtype"], c["center"], c["scale"])


def as_bytes(tabs):
    return tuple(np.ascontiguousarray(t).tobytes() for t in tabs[:4])


def run(la, c, lengths, memory, acc=None):
    """-> the four tables of case `c` fed in chunks of `lengths`; with `acc`, on that accumulator (which is left open)"""
    own = acc is None
    if own:
        acc = new(la, c)
    cases.feed(la, acc, c["x"].astype(acc.np_dtype), lengths, memory)
    assert acc.n_draws == c["n"]
    tabs = acc.tables()
    assert tabs[4] == c["n"]
    res = acc.result()
    assert as_bytes([res[k] for k in ("moment", "chain_outer", "sum", "chain_sums")]) == as_bytes(tabs) and res["nobs"] == c["n"] * c["C"]
    if own:
        acc.free()
    return tabs[:4], res


def check_case(la, name, dtype, report=None):
    c = cases.case(name, dtype)
    ref = reference(name, dtype)
    first = None
    for label, lengths, memory in cases.chunkings(c["n"]):
        tabs, res = run(la, c, lengths, memory)
        ratio, bad = cr.compare(tabs, ref)
        print(f"[cov] {name} {dtype} {label} ({memory}): error / bound {ratio:.3e}")
        if report is not None:
            report(name, dtype, label, memory, ratio)
        assert not bad, (name, dtype, label, memory, bad)
        if first is None:
            first = as_bytes(tabs)
            derived_figures(c, ref, res)
        assert as_bytes(tabs) == first, (name, dtype, label, memory, "bytes differ from the first feeding")
    return first


def derived_figures(c, ref, res):
    """cov, cor, mean of the device's tables against NumPy on the draws, on the finite coordinates, within the propagated bounds; the
    non-finite coordinates have non-finite rows and columns and leave the others alone."""
    J = np.flatnonzero(ref["finite"])
    bad = np.flatnonzero(~ref["finite"])
    assert not np.isfinite(res["cov"][bad]).any() and not np.isfinite(res["cov"][:, bad]).any() and not np.isfinite(res["mean"][bad]).any()
    if J.size == 0:
        return
    ix = np.ix_(J, J)
    if c["name"].endswith("_same"):
        N = c["n"] * c["C"]
        tol = 2.02 * ref["tol_moment"] / np.outer(c["scale"], c["scale"]) / (N - 1)  # M and s s^T / N, each within the moment's bound
        assert np.all(np.abs(res["cov"]) <= tol) and np.all(np.isnan(res["cor"]))  # (0.25 N and (0.5 N)^2 / N are exact: the variance is 0)
        return
    want = cr.derived(c["x"][:, :, J])
    tol = cr.derived_bounds(ref, J, c["center"], c["scale"])
    for key in ("mean", "cov") + (("cor",) if c["n"] * c["C"] > 1 else ()):
        got = res[key][ix] if res[key].ndim == 2 else res[key][J]
        err, t = np.abs(got - want[key]), 2.0 * tol["tol_" + key]
        assert np.all(err <= t), (c["name"], c["dtype"], key, float(np.max(err / t)))


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_table_against_the_reference_and_every_feeding_gives_the_same_bytes(la, name, dtype):
    check_case(la, name, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_reset_repeats_the_bytes_and_more_draws_may_follow_a_result(la, dtype):
    for name in ("C37_p8_n64", "C3_p128_n16", "C130_p3_n601"):
        c = cases.case(name, dtype)
        x = c["x"].astype(dtype)
        acc = new(la, c)
        t0 = acc.tables()
        assert all(np.all(np.isnan(t)) for t in t0[:4]) and t0[4] == 0 and acc.n_draws == 0
        a, _ = run(la, c, [c["n"]], "host", acc)
        acc.reset()
        assert acc.n_draws == 0 and all(np.all(np.isnan(t)) for t in acc.tables()[:4])
        half = c["n"] // 2
        acc.update(x[:half])
        part = acc.tables()  # a result in the middle of the run changes nothing
        assert part[4] == half
        ratio, bad = cr.compare(part[:4], cr.tables(c["x"][:half], c["center"], c["scale"]))
        assert not bad, (name, dtype, bad)
        acc.update(x[half:])
        assert as_bytes(acc.tables()) == as_bytes(a), name
        acc.free()
        with pytest.raises(la.LogregHipError, match="freed"):
            acc.update(x[:1])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_both_builds_give_the_same_bytes(la, dtype):
    """The production library and the second build (tests/altlib.py: default scheduler, SLP on): the arithmetic is spelled out (explicit
    fma, contraction off), so flags may not change a result."""
    from logreg_amd import _lib
    import altlib
    for name in ("C37_p8_n64", "C5_p20_n200", "C3_p128_n16", "C130_p3_n601"):
        c = cases.case(name, dtype)
        label, lengths, memory = cases.chunkings(c["n"])[4]  # uneven, device memory
        a, _ = run(la, c, lengths, memory)
        L = altlib.install()
        try:
            _lib.bind_covariance(L)
            assert _lib.load() is L
            b, _ = run(la, c, lengths, memory)
        finally:
            altlib.uninstall()
            _lib.bind_covariance(_lib.load())
        assert as_bytes(a) == as_bytes(b), name


def test_c_abi_refuses_bad_arguments_with_a_reason(la):
    import ctypes as C
    from logreg_amd import _lib
    L = _lib.load_covariance()
    h = C.c_void_p()
    ctr, scl = np.zeros(3), np.ones(3)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    big, zero, inf, nan = np.ones(129), np.array([1.0, 0.0, 1.0]), np.array([1.0, np.inf, 1.0]), np.array([0.0, np.nan, 0.0])
    for args, word in (((0, 0, 0, 3, ptr(ctr), ptr(scl)), "positive"), ((0, 0, 5, 0, ptr(ctr), ptr(scl)), "positive"), ((0, 0, 5, 129, ptr(big), ptr(big)), "1..128"),
                       ((0, 7, 5, 3, ptr(ctr), ptr(scl)), "dtype"), ((0, 0, 5, 3, ptr(ctr), ptr(zero)), "scale > 0"),
                       ((0, 0, 5, 3, ptr(ctr), ptr(inf)), "finite"), ((0, 0, 5, 3, ptr(nan), ptr(scl)), "finite"),
                       ((0, 0, 5, 3, None, ptr(scl)), "NULL"), ((0, 0, 5, 3, ptr(ctr), None), "NULL")):
        assert L.lr_cov_create(*args, C.byref(h)) != 0 and word in L.lr_last_error().decode(), args
    assert L.lr_cov_create(0, 0, 5, 3, ptr(ctr), ptr(scl), None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_cov_create(0, 1, 5, 3, ptr(ctr), ptr(scl), C.byref(h)) == 0
    x = np.zeros((2, 5, 3))
    assert L.lr_cov_accumulate(h, None, 2, 0, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_cov_accumulate(None, x.ctypes.data, 2, 0, None) != 0
    assert L.lr_cov_accumulate(h, x.ctypes.data, 0, 0, None) != 0 and "positive" in L.lr_last_error().decode()
    assert L.lr_cov_result(None, None, None, None, None, None) != 0 and L.lr_cov_reset(None) != 0
    n = C.c_int64(-1)
    M, S = np.ones((3, 3)), np.ones((5, 3))
    assert L.lr_cov_result(h, M.ctypes.data, None, None, S.ctypes.data, C.byref(n)) == 0 and n.value == 0  # refused calls left it empty
    assert np.all(np.isnan(M)) and np.all(np.isnan(S))
    L.lr_cov_destroy(h)
    L.lr_cov_destroy(None)


def golden(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def pima_setup(la, dtype, kind):
    d, mp = golden("pima_xy.json"), golden("map.json")
    X, y = np.array(d["X"]), np.array(d["y"])
    model = la.LogReg(X, y, np.array(mp["pscale"]), dtype=dtype)
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    if kind == "hmc":
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
    else:
        kern = la.nutsKernel(model.lpost, model.glp, eps=1e-3, dmm=1 / pre, max_depth=5)
    init = np.array(mp["map"]) + 0.01 * np.random.default_rng(5).standard_normal((64, 8))
    sd = np.array([1.0, 0.06, 0.007, 0.02, 0.02, 0.04, 0.65, 0.02])  # roughly the posterior's
    center, scale = la.covariance_scaling(np.array(mp["map"]), sd)
    return model, kern, init, center, scale


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")  # (strings and counts: plain equality)


@pytest.mark.parametrize("dtype,kind", [("float32", "hmc"), ("float64", "hmc"), ("float32", "nuts")])
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype, kind):
    model, kern, init, center, scale = pima_setup(la, dtype, kind)
    kw = dict(thin=2, iters=40, verb=False, seed=99, chunk=7)
    mat, info = la.mcmc(init, kern, return_info=True, **kw)  # summary_only=False: the kept block of the same seed
    one = la.Covariance(64, 8, dtype, center, scale).update(mat)
    want = one.result()
    ref = cr.tables(mat.astype(np.float64), center, scale)
    ratio, bad = cr.compare(one.tables()[:4], ref)
    print(f"[cov] mcmc {kind} {dtype}: error / bound {ratio:.3e}")
    assert not bad, bad
    assert want["nobs"] == 40 * 64 and np.all(np.isfinite(want["cov"])) and np.all(np.abs(want["cor"]) <= 1 + 1e-12)
    # summary_only: the blocks never reach the host, the accumulator sees the same draws
    plain = la.mcmc(init, kern, summary_only=True, **kw)
    acc = la.Covariance(64, 8, dtype, center, scale)
    res = la.mcmc(init, kern, summary_only=True, covariance=acc, **kw)
    assert set(res) == set(plain) | {"covariance"} and all(same(plain[k], res[k]) for k in plain)
    assert np.array_equal(plain["state"], info["state"])
    assert acc.n_draws == 40 and same(res["covariance"], want)
    assert as_bytes(acc.tables()) == as_bytes(one.tables())
    # the matrix path, with return_info=True: the info dict gains it
    acc2 = la.Covariance(64, 8, dtype, center, scale)
    mat2, info2 = la.mcmc(init, kern, return_info=True, covariance=acc2, **kw)
    assert mat.tobytes() == mat2.tobytes() and set(info2) == set(info) | {"covariance"} and all(same(info[k], info2[k]) for k in info)
    assert same(info2["covariance"], want) and as_bytes(acc2.tables()) == as_bytes(one.tables())
    for q in (one, acc, acc2):
        q.free()
    model.close()


def test_a_host_block_one_step_longer_than_a_staging_piece_gives_the_bytes_of_two_updates(la):
    """The one path no case above reaches: a host block that does not fit one staging piece.  One `update` with a step more than a
    piece is the launch sequence of two `update`s cut at the piece boundary, so the bytes are the same."""
    # a host block is staged in pieces of max(1, 256 MB / (C p esize)) time steps: 256 MB / (8192 x 64 x 8 bytes) = 64 steps.  (A change of
    # the 256 MB needs another shape here.)
    Cn, p, piece = 8192, 64, 64
    x = np.random.default_rng(12).standard_normal((piece + 1, Cn, p))
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        acc = la.Covariance(Cn, p, "float64", center=np.zeros(p), scale=np.ones(p))
        t0 = 0
        for k in cuts:
            acc.update(x[t0:t0 + k])
            t0 += k
        assert acc.n_draws == piece + 1
        out.append(acc.tables())
        acc.free()
    M, Q, s, S, n = out[0]
    assert n == piece + 1 and np.all(np.isfinite(M)) and np.all(np.diag(M) > 0) and np.allclose(S, x.sum(axis=0), rtol=0, atol=1e-11)
    assert as_bytes(out[0]) == as_bytes(out[1])


def measure():
    """Print the error / bound ratio of every case and feeding, and the largest per dtype (profiles/r16_cov.txt)."""
    import logreg_amd as la
    worst = {}

    def report(name, dtype, label, memory, ratio):
        worst[dtype] = max(worst.get(dtype, 0.0), ratio)
    for name in cases.NAMES:
        for dtype in cases.DTYPES:
            check_case(la, name, dtype, report)
    for dtype, v in worst.items():
        print(f"FIGURE largest error / bound {dtype} {v:.3e}")


if __name__ == "__main__":
    import os
    if sys.argv[1:] != ["--measure"]:
        sys.exit("usage: python tests/test_gpu_cov.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
