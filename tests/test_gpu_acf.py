"""The autocorrelation / Geyer-ESS accumulator on the GPU (include/logreg_hip_acf.h, csrc/lr_acf.h) against tests/acf_reference.py.

Every row of `sums` and every entry of `ess_chain` of every case of tests/acf_cases.py (both dtypes) is compared with the independent
long-double reference on the same dtype-rounded input, within the forward-error bounds the reference derives from the input alone
(tests/acf_reference.py: nothing here is measured on the kernel); the capped and NaN counts exactly; NaN exactly where the reference
has it.  Across all feedings (one call, chunks of 1, 7, K, K + 1, uneven; host and device memory), a repeat after reset() and the
second build of the library the bytes are identical.  `python tests/test_gpu_acf.py --measure` prints the error / bound ratios
(profiles/r11_acf.txt).
"""
import faulthandler
import sys

import numpy as np
import pytest

import acf_cases as cases
import acf_reference as ar

pytestmark = pytest.mark.gpu
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        c = cases.case(name, dtype)
        _REF[(name, dtype)] = ar.reference(c["x"], c["K"])
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


def run(la, c, lengths, memory, ac=None):
    """-> (sums, ess_chain) of case `c` fed in chunks of `lengths`; with `ac`, on that accumulator (which is left open)"""
    own = ac is None
    if own:
        ac = la.Autocorr(c["C"], c["p"], c["dtype"], max_lag=c["K"])
    cases.feed(la, ac, c["x"].astype(ac.np_dtype), lengths, memory)
    assert ac.n_draws == c["n"]
    out = ac.sums()
    if own:
        ac.free()
    return out


def check_case(la, name, dtype, report=None):
    c = cases.case(name, dtype)
    ref = reference(name, dtype)
    assert np.nanmin(ref["margin"]) >= 1e3 if ref["margin"].size else True  # (the condition on the inputs: tests/test_acf_cpu.py)
    first = None
    for label, lengths, memory in cases.chunkings(c["n"], c["K"]):
        sums, ess = run(la, c, lengths, memory)
        ratio, bad = ar.compare(sums, ess, ref)
        print(f"[acf] {name} {dtype} {label} ({memory}): error / bound {ratio:.3e}")
        if report is not None:
            report(name, dtype, label, memory, ratio)
        assert not bad, (name, dtype, label, memory, bad)
        if first is None:
            first = (sums.tobytes(), ess.tobytes())
        assert (sums.tobytes(), ess.tobytes()) == first, (name, dtype, label, memory, "bytes differ from the first feeding")
    return first


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_entry_against_the_reference_and_every_feeding_gives_the_same_bytes(la, name, dtype):
    check_case(la, name, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_reset_repeats_the_bytes_and_more_draws_may_follow_a_result(la, dtype):
    for name in ("C37_p8_n64_K63", "C5_p3_n601_K255", "C130_p8_n200_K7"):
        c = cases.case(name, dtype)
        x = c["x"].astype(dtype)
        ac = la.Autocorr(c["C"], c["p"], dtype, max_lag=c["K"])
        empty, ess0 = ac.sums()
        assert np.all(np.isnan(empty)) and np.all(np.isnan(ess0)) and ac.n_draws == 0
        a = run(la, c, [c["n"]], "host", ac)
        ac.reset()
        assert ac.n_draws == 0 and np.all(np.isnan(ac.sums()[0]))
        half = c["n"] // 2
        ac.update(x[:half])
        part = ac.sums()  # a result in the middle of the run changes nothing
        ratio, bad = ar.compare(*part, ar.reference(c["x"][:half], c["K"]))
        assert not bad, (name, dtype, bad)
        ac.update(x[half:])
        b = ac.sums()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
        res = ac.result()
        assert res["n"] == c["n"] and res["chains"] == c["C"] and res["max_lag"] == c["K"] and res["acf"].shape == (c["K"] + 1, c["p"])
        assert np.array_equal(res["ess"], b[0][0], equal_nan=True) and np.array_equal(res["ess_chain"], b[1], equal_nan=True)
        ac.free()
        with pytest.raises(la.LogregHipError, match="freed"):
            ac.update(x[:1])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_both_builds_give_the_same_bytes(la, dtype):
    """The production library and the second build (tests/altlib.py: default scheduler, SLP on): the arithmetic is spelled out (explicit
    fma), so flags may not change a result."""
    from logreg_amd import _lib
    import altlib
    for name in ("C37_p8_n64_K63", "C5_p3_n601_K255", "C130_p8_n200_K7", "C37_p1_n601_K63", "C5_p20_n200_K63"):
        c = cases.case(name, dtype)
        label, lengths, memory = cases.chunkings(c["n"], c["K"])[6]  # uneven, device memory
        a = run(la, c, lengths, memory)
        L = altlib.install()
        try:
            _lib.bind_acf(L)
            assert _lib.load() is L
            b = run(la, c, lengths, memory)
        finally:
            altlib.uninstall()
            _lib.bind_acf(_lib.load())
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name


def test_c_abi_refuses_bad_arguments_with_a_reason(la):
    import ctypes as C
    from logreg_amd import _lib
    L = _lib.load_acf()
    h = C.c_void_p()
    for args, word in (((0, 0, 5, 3, 64), "odd"), ((0, 0, 5, 3, 257), "odd"), ((0, 0, 0, 3, 63), "positive"), ((0, 0, 5, 0, 63), "positive"),
                       ((0, 7, 5, 3, 63), "dtype")):
        assert L.lr_acf_create(*args, C.byref(h)) != 0 and word in L.lr_last_error().decode(), args
    assert L.lr_acf_create(0, 0, 5, 3, 63, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_acf_create(0, 1, 5, 3, 63, C.byref(h)) == 0
    x = np.zeros((2, 5, 3))
    assert L.lr_acf_accumulate(h, None, 2, 0, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_acf_accumulate(None, x.ctypes.data, 2, 0, None) != 0
    assert L.lr_acf_accumulate(h, x.ctypes.data, 0, 0, None) != 0 and "positive" in L.lr_last_error().decode()
    assert L.lr_acf_result(h, None, None, None) != 0 and L.lr_acf_reset(None) != 0
    n = C.c_int64(-1)
    sums = np.empty((67, 3))
    assert L.lr_acf_result(h, sums.ctypes.data, None, C.byref(n)) == 0 and n.value == 0 and np.all(np.isnan(sums))  # refused calls left it empty
    L.lr_acf_destroy(h)
    L.lr_acf_destroy(None)


def pima_setup(la, dtype, kind):
    d = cases_golden("pima_xy.json")
    mp = cases_golden("map.json")
    X, y = np.array(d["X"]), np.array(d["y"])
    model = la.LogReg(X, y, np.array(mp["pscale"]), dtype=dtype)
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    if kind == "hmc":
        kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
    else:
        kern = la.nutsKernel(model.lpost, model.glp, eps=1e-3, dmm=1 / pre, max_depth=5)
    init = np.array(mp["map"]) + 0.01 * np.random.default_rng(5).standard_normal((37, 8))
    return model, kern, init


def cases_golden(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")  # (strings and counts: plain equality)


@pytest.mark.parametrize("dtype,kind", [("float32", "hmc"), ("float64", "hmc"), ("float32", "nuts")])
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype, kind):
    model, kern, init = pima_setup(la, dtype, kind)
    kw = dict(thin=2, iters=50, verb=False, seed=99, chunk=7)
    mat, info = la.mcmc(init, kern, return_info=True, **kw)
    ac = la.Autocorr(37, 8, dtype)
    mat2, info2 = la.mcmc(init, kern, return_info=True, autocorr=ac, **kw)
    assert mat.shape == (50, 37, 8) and mat.tobytes() == mat2.tobytes()
    assert set(info2) == set(info) | {"autocorr"} and all(same(info[k], info2[k]) for k in info)
    one = la.Autocorr(37, 8, dtype).update(mat)  # the returned matrix in one call
    want = one.result()
    assert ac.n_draws == 50 and same(ac.result(), want) and same(info2["autocorr"], want)
    assert ac.sums()[0].tobytes() == one.sums()[0].tobytes() and ac.sums()[1].tobytes() == one.sums()[1].tobytes()
    ratio, bad = ar.compare(*one.sums(), ar.reference(mat.astype(np.float64), 63))  # (K = 63 > n / 2: nothing is capped)
    print(f"[acf] mcmc {kind} {dtype}: error / bound {ratio:.3e}")
    assert not bad, bad
    assert np.all(want["capped"] == 0) and np.all(want["nan_chains"] == 0) and np.all(want["ess"] > 0)
    assert np.allclose(want["ess"], la.ess_pooled(mat.astype(np.float64), max_chains=None), rtol=1e-9, atol=0)
    # summary_only: the blocks never reach the host, the accumulator sees the same draws
    plain = la.mcmc(init, kern, summary_only=True, **kw)
    ac3 = la.Autocorr(37, 8, dtype)
    with_ac = la.mcmc(init, kern, summary_only=True, autocorr=ac3, **kw)
    assert set(with_ac) == set(plain) | {"autocorr"} and all(same(plain[k], with_ac[k]) for k in plain)
    assert same(with_ac["autocorr"], want) and ac3.sums()[0].tobytes() == one.sums()[0].tobytes()
    assert np.array_equal(plain["state"], info["state"])
    for q in (ac, one, ac3):
        q.free()
    model.close()


def test_a_host_block_one_step_longer_than_a_staging_piece_gives_the_bytes_of_two_updates(la):
    """The one path no case above reaches: a host block that does not fit one staging piece.  One `update` with a step more than a
    piece is the launch sequence of two `update`s cut at the piece boundary, so the bytes are the same."""
    # a host block is staged in pieces of max(1, 256 MB / (C p esize)) time steps: 256 MB / (8192 x 64 x 8 bytes) = 64 steps.  (A change of
    # the 256 MB needs another shape here.)
    Cn, p, piece = 8192, 64, 64
    x = np.random.default_rng(11).standard_normal((piece + 1, Cn, p))
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        ac = la.Autocorr(Cn, p, "float64", max_lag=1)
        t0 = 0
        for k in cuts:
            ac.update(x[t0:t0 + k])
            t0 += k
        assert ac.n_draws == piece + 1
        out.append(ac.sums())
        ac.free()
    assert np.all(np.isfinite(out[0][0][3:])) and np.all(out[0][0][3] > 0)
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def measure():
    """Print the error / bound ratio of every case and feeding, and the largest per dtype (profiles/r11_acf.txt)."""
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
        sys.exit("usage: python tests/test_gpu_acf.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
