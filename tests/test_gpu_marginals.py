"""The marginals accumulator on the GPU (include/logreg_hip_marginals.h, csrc/lr_marginals.h) against tests/marginals_reference.py.

For every case of tests/marginals_cases.py (both dtypes) and every feeding (one call, chunks of 1, of 7, uneven; host and device memory):
the counts EQUAL the reference's, min / max equal, the power sums (rows 2..5) and mean, variance, skewness and kurtosis lie within the
forward-error bounds the reference derives from the input alone (nothing here is measured on the kernel), every figure is finite
exactly where the reference's is, and the bytes of (counts, table) are identical across all feedings, a repeat after reset() and the
second build of the library.  `python tests/test_gpu_marginals.py --measure` prints the error / bound ratios
(profiles/r12_marginals.txt).
"""
import faulthandler
import sys

import numpy as np
import pytest

import marginals_cases as cases
import marginals_reference as mr

pytestmark = pytest.mark.gpu
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = cases.case(name, dtype)
        _REF[(name, dtype)] = mr.reference(c["x"], c["lo"], c["hi"], c["B"])
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
    return la.Marginals(c["C"], c["p"], c["dtype"], c["lo"], c["hi"], bins=c["B"])


def run(la, c, lengths, memory, mg=None):
    """-> (counts, table, result dict) of case `c` fed in chunks of `lengths`; with `mg`, on that accumulator (which is left open)"""
    own = mg is None
    if own:
        mg = new(la, c)
    cases.feed(la, mg, c["x"].astype(mg.np_dtype), lengths, memory)
    assert mg.n_draws == c["n"]
    counts, table = mg.counts_table()
    res = mg.result()
    assert np.array_equal(res["columns"], counts) and res["table"].tobytes() == table.tobytes() and res["nobs"] == c["n"] * c["C"]
    if own:
        mg.free()
    return counts, table, res


def check_case(la, name, dtype, report=None):
    c = cases.case(name, dtype)
    ref = reference(name, dtype)
    first = None
    for label, lengths, memory in cases.chunkings(c["n"]):
        counts, table, res = run(la, c, lengths, memory)
        ratio, bad = mr.compare(counts, table, res, ref)
        print(f"[marginals] {name} {dtype} {label} ({memory}): error / bound {ratio:.3e}")
        if report is not None:
            report(name, dtype, label, memory, ratio)
        assert not bad, (name, dtype, label, memory, bad)
        if first is None:
            first = (counts.tobytes(), table.tobytes())
        assert (counts.tobytes(), table.tobytes()) == first, (name, dtype, label, memory, "bytes differ from the first feeding")
    return first


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_entry_against_the_reference_and_every_feeding_gives_the_same_bytes(la, name, dtype):
    check_case(la, name, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_reset_repeats_the_bytes_and_more_draws_may_follow_a_result(la, dtype):
    for name in ("C37_p8_n64_B64", "C3_p128_n16_B1024", "C130_p3_n601_B1024"):
        c = cases.case(name, dtype)
        x = c["x"].astype(dtype)
        mg = new(la, c)
        counts0, table0 = mg.counts_table()
        assert np.all(counts0 == 0) and np.all(np.isnan(table0)) and mg.n_draws == 0
        a = run(la, c, [c["n"]], "host", mg)
        mg.reset()
        assert mg.n_draws == 0 and np.all(mg.counts_table()[0] == 0) and np.all(np.isnan(mg.counts_table()[1]))
        half = c["n"] // 2
        mg.update(x[:half])
        part = mg.counts_table()  # a result in the middle of the run changes nothing
        ratio, bad = mr.compare(*part, None, mr.reference(c["x"][:half], c["lo"], c["hi"], c["B"]))
        assert not bad, (name, dtype, bad)
        mg.update(x[half:])
        b = mg.counts_table()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
        mg.free()
        with pytest.raises(la.LogregHipError, match="freed"):
            mg.update(x[:1])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_both_builds_give_the_same_bytes(la, dtype):
    """The production library and the second build (tests/altlib.py: default scheduler, SLP on): the arithmetic is spelled out (explicit
    fma, contraction off), so flags may not change a result."""
    from logreg_amd import _lib
    import altlib
    for name in ("C37_p8_n64_B64", "C5_p20_n200_B256", "C3_p128_n16_B1024", "C130_p3_n601_B1024"):
        c = cases.case(name, dtype)
        label, lengths, memory = cases.chunkings(c["n"])[4]  # uneven, device memory
        a = run(la, c, lengths, memory)
        L = altlib.install()
        try:
            _lib.bind_marginals(L)
            assert _lib.load() is L
            b = run(la, c, lengths, memory)
        finally:
            altlib.uninstall()
            _lib.bind_marginals(_lib.load())
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name


def test_a_coordinate_without_a_number_has_no_min_and_max(la):
    x = np.zeros((5, 3, 2))
    x[:, :, 1] = np.nan
    mg = la.Marginals(3, 2, "float64", [-1.0, -1.0], [1.0, 1.0], bins=4).update(x)
    counts, table = mg.counts_table()
    assert counts[1, 6] == 15 and counts[1, :6].sum() == 0 and counts[0, 3] == 15 and counts[0].sum() == 15
    assert np.all(table[:2, 0] == 0.0) and np.all(np.isnan(table[:, 1])) and np.all(table[2:, 0] == 0.0)
    from logreg_amd.marginals import quantile
    assert np.isnan(quantile(mg.result(), 0.5)[1]) and quantile(mg.result(), 0.5)[0] == 0.0
    mg.free()


def test_c_abi_refuses_bad_arguments_with_a_reason(la):
    import ctypes as C
    from logreg_amd import _lib
    L = _lib.load_marginals()
    h = C.c_void_p()
    lo, hi = np.zeros(3), np.ones(3)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    for args, word in (((0, 0, 5, 3, 0, ptr(lo), ptr(hi)), "bins"), ((0, 0, 5, 3, 1025, ptr(lo), ptr(hi)), "bins"), ((0, 0, 0, 3, 8, ptr(lo), ptr(hi)), "positive"),
                       ((0, 0, 5, 0, 8, ptr(lo), ptr(hi)), "positive"), ((0, 7, 5, 3, 8, ptr(lo), ptr(hi)), "dtype"), ((0, 0, 5, 3, 8, ptr(hi), ptr(lo)), "lo < hi"),
                       ((0, 0, 5, 3, 8, ptr(lo), ptr(np.array([1.0, np.inf, 1.0]))), "finite"), ((0, 0, 5, 3, 8, None, ptr(hi)), "NULL")):
        assert L.lr_marg_create(*args, C.byref(h)) != 0 and word in L.lr_last_error().decode(), args
    assert L.lr_marg_create(0, 0, 5, 3, 8, ptr(lo), ptr(hi), None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_marg_create(0, 1, 5, 3, 8, ptr(lo), ptr(hi), C.byref(h)) == 0
    x = np.zeros((2, 5, 3))
    assert L.lr_marg_accumulate(h, None, 2, 0, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_marg_accumulate(None, x.ctypes.data, 2, 0, None) != 0
    assert L.lr_marg_accumulate(h, x.ctypes.data, 0, 0, None) != 0 and "positive" in L.lr_last_error().decode()
    assert L.lr_marg_result(None, None, None, None) != 0 and L.lr_marg_reset(None) != 0
    n = C.c_int64(-1)
    counts, table = np.ones((3, 11), dtype=np.uint64), np.empty((6, 3))
    assert L.lr_marg_result(h, counts.ctypes.data, table.ctypes.data, C.byref(n)) == 0 and n.value == 0  # refused calls left it empty
    assert np.all(counts == 0) and np.all(np.isnan(table))
    L.lr_marg_destroy(h)
    L.lr_marg_destroy(None)


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
    init = np.array(mp["map"]) + 0.01 * np.random.default_rng(5).standard_normal((37, 8))
    sd = np.array([1.0, 0.06, 0.007, 0.02, 0.02, 0.04, 0.65, 0.02])  # roughly the posterior's; the start is 0.01 off the mode, so some draws leave the grid
    lo, hi = la.marginal_grid(np.array(mp["map"]), sd, width=4.0)
    return model, kern, init, lo, hi


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")  # (strings and counts: plain equality)


@pytest.mark.parametrize("dtype,kind", [("float32", "hmc"), ("float64", "hmc"), ("float32", "nuts")])
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype, kind):
    model, kern, init, lo, hi = pima_setup(la, dtype, kind)
    kw = dict(thin=2, iters=40, verb=False, seed=99, chunk=7)
    mat, info = la.mcmc(init, kern, return_info=True, **kw)
    one = la.Marginals(37, 8, dtype, lo, hi).update(mat)  # the matrix of the same seeded run, in one call
    want = one.result()
    ref = mr.reference(mat.astype(np.float64), lo, hi, 256)
    ratio, bad = mr.compare(*one.counts_table(), want, ref)
    print(f"[marginals] mcmc {kind} {dtype}: error / bound {ratio:.3e}")
    assert not bad, bad
    assert want["nobs"] == 40 * 37 and np.all(want["nan"] == 0) and np.all(want["counts"].sum(axis=1) + want["underflow"] + want["overflow"] == 40 * 37)
    # summary_only: the blocks never reach the host, the accumulator sees the same draws
    plain = la.mcmc(init, kern, summary_only=True, **kw)
    mg = la.Marginals(37, 8, dtype, lo, hi)
    res = la.mcmc(init, kern, summary_only=True, marginals=mg, **kw)
    assert set(res) == set(plain) | {"marginals"} and all(same(plain[k], res[k]) for k in plain)
    assert np.array_equal(plain["state"], info["state"])
    assert mg.n_draws == 40 and same(res["marginals"], want)
    assert mg.counts_table()[0].tobytes() == one.counts_table()[0].tobytes() and mg.counts_table()[1].tobytes() == one.counts_table()[1].tobytes()
    # the matrix path, with return_info=True: the info dict gains it
    mg2 = la.Marginals(37, 8, dtype, lo, hi)
    mat2, info2 = la.mcmc(init, kern, return_info=True, marginals=mg2, **kw)
    assert mat.tobytes() == mat2.tobytes() and set(info2) == set(info) | {"marginals"} and all(same(info[k], info2[k]) for k in info)
    assert same(info2["marginals"], want) and mg2.counts_table()[1].tobytes() == one.counts_table()[1].tobytes()
    for q in (one, mg, mg2):
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
        mg = la.Marginals(Cn, p, "float64", lo=np.full(p, -3.0), hi=np.full(p, 3.0), bins=8)
        t0 = 0
        for k in cuts:
            mg.update(x[t0:t0 + k])
            t0 += k
        assert mg.n_draws == piece + 1
        out.append(mg.counts_table())
        mg.free()
    counts, table = out[0]
    assert np.all(counts.sum(axis=1) == (piece + 1) * Cn) and np.all(counts[:, 1:9] > 0) and np.all(np.isfinite(table))
    assert counts.tobytes() == out[1][0].tobytes() and table.tobytes() == out[1][1].tobytes()


def measure():
    """Print the error / bound ratio of every case and feeding, and the largest per dtype (profiles/r12_marginals.txt)."""
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
        sys.exit("usage: python tests/test_gpu_marginals.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
