"""The rank-diagnostics accumulator on the GPU (include/logreg_hip_rank.h, csrc/lr_rank.h) against tests/rank_reference.py.

Ranks (plain and folded) are compared as integers at every shape and input of tests/rank_cases.py; z against scipy's ndtri on those
ranks; the statistics against the float64 reference, once fed the device's own z and once end to end from the raw draws, with the
number of pairs kept and the capped flags equal.  The bounds on z and on the statistics are 8 x the largest error measured over these
cases and every other comparison of this file (`python tests/test_gpu_rank.py --measure`; profiles/r28_rank.txt section 1): the float64 reference is the yardstick.
Across all feedings (one call, single steps, uneven chunks, a block one step longer than a staging piece; host and device memory), a
repeat, a reset and the second build of the library the bytes are identical.
"""
import faulthandler
import json
import os
import sys

import numpy as np
import pytest
import scipy.special

import rank_cases as cases
import rank_reference as rr

pytestmark = pytest.mark.gpu
K = 63
FLOAT_ROWS = (0, 1, 2, 3, 4)     # rhat_bulk, rhat_tail, rhat, ess_bulk, ess_tail: within the bound
EXACT_ROWS = (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)  # flags, order statistics, counts, pairs kept: equal
# 8 x the largest error measured over the cases below on the device (profiles/r28_rank.txt section 1): relative to max(1, |z|) for z, relative for
# the statistics
BOUND = {"z": 8 * 9.667e-16, "from_z": 8 * 8.900e-15, "end_to_end": 8 * 8.900e-15}
_REF = {}
_MEASURED = None  # --measure: {what: the largest error seen} in place of the assertions


def within(what, err, *where):
    """err <= BOUND[what]; under --measure the error is recorded instead"""
    if _MEASURED is not None:
        _MEASURED[what] = max(_MEASURED.get(what, 0.0), err)
    else:
        assert err <= BOUND[what], (what, err, BOUND[what], *where)


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


def reference(shape, kind, dtype):
    """(x, table, margin, columns) of a case, computed once"""
    key = (shape, kind, dtype)
    if key not in _REF:
        x = cases.draws(shape, kind, dtype)
        T, margin = rr.table(x, K)
        x.setflags(write=False)
        _REF[key] = (x, T, margin)
    return _REF[key]


def fill(la, x, dtype, lengths=None, memory="host", max_steps=None):
    n, C, p = x.shape
    acc = la.RankDiagnostics(C, p, max_steps or n, dtype, max_lag=K)
    cases.feed(la, acc, x.astype(dtype), lengths or [n], memory)
    assert acc.n_draws == n
    return acc


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def same_exact_rows(T, R):
    for r in EXACT_ROWS:
        assert np.array_equal(T[r], R[r], equal_nan=True), (rr.ROWS[r], T[r], R[r])


# ---- ranks and z --------------------------------------------------------------------------------------------------------------------------------
def check_ranks(la, shape, dtype):
    n, C, p = shape
    S = n // 2 * 2 * C
    for kind in cases.RANK_KINDS:
        x = cases.draws(shape, kind, dtype)
        acc = fill(la, x, dtype)
        for j in range(p):
            x2, h = rr.used(x[:, :, j])
            med = rr.order_stats(x2)[0]
            for folded, want in ((False, rr.twice_ranks(x2)), (True, rr.twice_ranks(np.abs(x2 - med)))):
                r2, z = acc.ranks(j, folded=folded, with_z=True)
                assert r2.dtype == np.int64 and r2.shape == (2 * h, C) and np.array_equal(r2, want), (shape, kind, dtype, j, folded)
                zs = scipy.special.ndtri((r2 * 0.5 - 0.375) / (S + 0.25))
                err = float(np.max(np.abs(z - zs) / np.maximum(1.0, np.abs(zs))))
                print(f"[rank] z {shape} {kind} {dtype} j={j} folded={folded}: error {err:.3e}")
                within("z", err, shape, kind, dtype, j, folded)
        acc.free()


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_ranks_are_the_references_as_integers_and_z_is_ndtri_of_them(la, shape, dtype):
    check_ranks(la, shape, dtype)


# ---- the statistics -----------------------------------------------------------------------------------------------------------------------------
def check_statistics(la, shape, dtype):
    n, C, p = shape
    for kind in cases.STAT_KINDS:
        x, R, margin = reference(shape, kind, dtype)
        assert np.all(margin > 1e-6), (shape, kind, dtype, margin)  # (the condition on the inputs: no pair of the scan within 1e-6 of zero)
        acc = fill(la, x, dtype)
        T = acc.table()
        z = [acc.ranks(j, with_z=True)[1] for j in range(p)]
        zf = [acc.ranks(j, folded=True, with_z=True)[1] for j in range(p)]
        acc.free()
        Rz, _ = rr.table(x, K, z=z, zf=zf)  # the reference fed the device's own z
        same_exact_rows(T, R)
        same_exact_rows(T, Rz)
        e_z, e_all = rel(T[list(FLOAT_ROWS)], Rz[list(FLOAT_ROWS)]), rel(T[list(FLOAT_ROWS)], R[list(FLOAT_ROWS)])
        print(f"[rank] statistics {shape} {kind} {dtype}: error from the device's z {e_z:.3e}, end to end {e_all:.3e}")
        within("from_z", e_z, shape, kind, dtype)
        within("end_to_end", e_all, shape, kind, dtype)
        if shape[0] >= 64:  # (nine steps give no stable figure)
            assert np.all(np.isfinite(T[list(FLOAT_ROWS)])) and np.all(T[3] > 0) and np.all(T[4] > 0)


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_statistics_against_the_reference_from_the_devices_z_and_end_to_end(la, shape, dtype):
    check_statistics(la, shape, dtype)


def test_the_two_cases_the_classical_rhat_is_blind_to(la):
    """One chain three times wider; Cauchy chains with one shifted by 3 (8 chains x 400 draws): classical split-R-hat < 1.01, rank R-hat > 1.05
    -- on the device as in the reference, and `diagnostics.split_rhat` agrees about the classical figure."""
    rng = np.random.default_rng(0)
    wide = rng.standard_normal((400, 8))
    wide[:, 0] *= 3
    cauchy = rng.standard_cauchy((400, 8))
    cauchy[:, 0] += 3
    x = np.stack([wide, cauchy], axis=2)
    acc = fill(la, x, "float64")
    res = acc.result()
    acc.free()
    R, _ = rr.table(x, K)
    classical = la.split_rhat(x)
    assert np.all(classical < 1.01) and abs(classical[0] - rr.classical_split_rhat(wide)) < 1e-12
    assert res["rhat_tail"][0] > 1.05 and res["rhat_bulk"][0] < 1.01 and res["rhat_bulk"][1] > 1.05 and np.all(res["rhat"] > 1.05)
    within("end_to_end", rel(res["table"][list(FLOAT_ROWS)], R[list(FLOAT_ROWS)]), "the blind cases")
    same_exact_rows(res["table"], R)


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_a_nan_or_an_infinity_gives_nan_in_its_coordinate_alone_with_the_count(la, dtype):
    shape = (64, 5, 3)
    x, R, _ = reference(shape, "smooth", dtype)
    acc = fill(la, x, dtype)
    clean = acc.table()
    acc.free()
    for j, bad in ((0, [np.nan]), (1, [np.inf]), (2, [-np.inf, np.nan, np.inf]), (1, [-np.nan])):
        y = x.copy()
        for i, v in enumerate(bad):
            y[7 + 11 * i, (2 + i) % 5, j] = v
        acc = fill(la, y, dtype)
        T = acc.table()
        for jj in range(3):
            r2 = acc.ranks(jj)
            assert r2.min() >= 2 and r2.max() <= 2 * 64 * 5  # (ranks of a coordinate with a NaN are still ranks: nothing reads out of bounds)
        acc.free()
        want = rr.table(y, K)[0]
        assert np.all(np.isnan(T[:11, j])) and np.all(np.isnan(T[12:, j])) and T[11, j] == len(bad) == want[11, j]
        others = [c for c in range(3) if c != j]
        assert T[:, others].tobytes() == clean[:, others].tobytes()
    # an infinity in the ignored odd last step does not count
    y = np.concatenate([x, x[:1]], axis=0)
    y[64, 0, 0] = np.inf
    acc = fill(la, y, dtype)
    assert acc.table().tobytes() == clean.tobytes() and acc.result()["n_used"] == 64 and acc.result()["n"] == 65
    acc.free()


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_fewer_than_four_steps_and_a_constant_column_give_nan(la, dtype):
    x = cases.draws((64, 5, 3), "equal", dtype)
    acc = fill(la, x, dtype)
    T, R = acc.table(), rr.table(x, K)[0]
    acc.free()
    assert np.all(np.isnan(T[:8, 0])) and np.all(np.isnan(T[12:, 0])) and T[11, 0] == 0 and np.all(T[8:11, 0] == 1.5)
    assert np.all(np.isfinite(T[:5, 1:]))
    within("end_to_end", rel(T[list(FLOAT_ROWS)], R[list(FLOAT_ROWS)]), "a constant column beside two smooth ones", dtype)
    same_exact_rows(T, R)
    acc = la.RankDiagnostics(5, 3, 8, dtype)
    assert np.all(np.isnan(acc.table()[:11])) and acc.n_draws == 0
    for n in (1, 2, 3):
        acc.update(x[n - 1:n].astype(dtype))
        T = acc.table()
        assert acc.n_draws == n and np.all(np.isnan(T[:11])) and np.all(np.isnan(T[12:])) and np.all(T[11] == 0), n
        assert acc.ranks(1).shape == (n // 2 * 2, 5)
    acc.update(x[3:4].astype(dtype))
    assert np.all(np.isfinite(acc.table()[8:11]))  # four steps: h = 2
    acc.free()


# ---- bytes --------------------------------------------------------------------------------------------------------------------------------------
def everything(acc):
    return acc.table().tobytes() + b"".join(acc.ranks(j, folded=f).tobytes() for j in range(acc.p) for f in (False, True))


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("shape", cases.SHAPES[:3])
def test_every_feeding_gives_the_same_bytes_and_results_leave_the_state_alone(la, shape, dtype):
    x, R, _ = reference(shape, "ar", dtype)
    first = None
    for label, lengths, memory in cases.feedings(shape[0]):
        acc = fill(la, x, dtype, lengths, memory, max_steps=shape[0] + 3)
        got = everything(acc)
        assert everything(acc) == got, (label, memory, "two results in a row differ")
        first = first or got
        assert got == first, (shape, dtype, label, memory, "bytes differ from the first feeding")
        acc.reset()
        assert acc.n_draws == 0 and np.all(np.isnan(acc.table()[:11]))
        half = shape[0] // 2
        acc.update(x[:half].astype(dtype))
        acc.table()  # a result in the middle of the run changes nothing
        acc.update(x[half:].astype(dtype))
        assert everything(acc) == first, (label, memory, "reset does not forget")
        with pytest.raises(ValueError, match="exceed max_steps"):
            acc.update(np.zeros((4, shape[1], shape[2])))
        assert everything(acc) == first
        acc.free()
        with pytest.raises(la.LogregHipError, match="freed"):
            acc.update(x[:1])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_both_builds_give_the_same_bytes(la, dtype):
    from logreg_amd import _lib
    import altlib
    for shape, kind in (((130, 67, 2), "ar"), ((258, 509, 2), "sticky"), ((64, 5, 3), "zeros")):
        x = cases.draws(shape, kind, dtype)
        acc = fill(la, x, dtype)
        a = everything(acc)
        acc.free()
        L = altlib.install()
        try:
            _lib.bind_rank(L)
            assert _lib.load() is L
            acc = fill(la, x, dtype)
            b = everything(acc)
            acc.free()
        finally:
            altlib.uninstall()
            _lib.bind_rank(_lib.load())
        assert a == b, (shape, kind)


def test_a_host_block_one_step_longer_than_a_staging_piece_gives_the_bytes_of_two_updates(la):
    """A host block is staged in pieces of max(1, 256 MB / (C p esize)) time steps: 256 MB / (8192 x 64 x 8 bytes) = 64 steps.  (A change of
    the 256 MB needs another shape here.)  64 coordinates of 2^19 draws are also more than one batch of coordinates."""
    Cn, p, piece = 8192, 64, 64
    x = np.random.default_rng(11).standard_normal((piece + 1, Cn, p))
    out = []
    for cuts in ([piece + 1], [piece, 1]):
        acc = la.RankDiagnostics(Cn, p, piece + 1, "float64", max_lag=7)
        t0 = 0
        for k in cuts:
            acc.update(x[t0:t0 + k])
            t0 += k
        assert acc.n_draws == piece + 1
        out.append((acc.table(), acc.ranks(p - 1)))
        acc.free()
    T, r2 = out[0]
    assert np.all(np.isfinite(T)) and np.all(T[2] < 1.01) and np.all(T[3] > 0.5 * piece * Cn)
    assert np.array_equal(r2, rr.twice_ranks(x[:piece, :, p - 1]))
    assert np.array_equal(T[8], np.sort(x[:piece].reshape(-1, p), axis=0)[[piece * Cn // 2 - 1, piece * Cn // 2]].mean(axis=0))
    assert T.tobytes() == out[1][0].tobytes() and r2.tobytes() == out[1][1].tobytes()


# ---- mcmc ----------------------------------------------------------------------------------------------------------------------------------------
def golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype):
    d, mp = golden("pima_xy.json"), golden("map.json")
    model = la.LogReg(np.array(d["X"]), np.array(d["y"]), np.array(mp["pscale"]), dtype=dtype)
    pre = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
    kern = la.hmcKernel(model.lpost, model.glp, eps=1e-3, l=20, dmm=1 / pre)
    init = np.array(mp["map"]) + 0.01 * np.random.default_rng(5).standard_normal((64, 8))
    kw = dict(thin=2, iters=40, verb=False, seed=99, chunk=7)
    # refused before anything runs
    for wrong, word in ((la.RankDiagnostics(63, 8, 40, dtype), "64 chains"), (la.RankDiagnostics(64, 8, 40, "float32" if dtype == "float64" else "float64"), "of float"),
                        (la.RankDiagnostics(64, 8, 40, dtype, device=1), "device"), (la.RankDiagnostics(64, 8, 39, dtype), "max_steps = 39"),
                        (la.Autocorr(64, 8, dtype), "must be a RankDiagnostics")):
        with pytest.raises(ValueError, match=word):
            la.mcmc(init, kern, rank=wrong, **kw)
        assert wrong.n_draws == 0 and wrong._h is None
    mat, info = la.mcmc(init, kern, return_info=True, **kw)
    rk = la.RankDiagnostics(64, 8, 40, dtype)
    mat2, info2 = la.mcmc(init, kern, return_info=True, rank=rk, **kw)
    assert mat.shape == (40, 64, 8) and mat.tobytes() == mat2.tobytes()
    assert set(info2) == set(info) | {"rank"} and all(same(info[k], info2[k]) for k in info)
    one = la.RankDiagnostics(64, 8, 40, dtype).update(mat)  # the kept draws by hand, in one call
    assert rk.n_draws == 40 and everything(rk) == everything(one) and same(info2["rank"], one.result())
    R, _ = rr.table(mat.astype(np.float64), K)
    same_exact_rows(one.table(), R)
    within("end_to_end", rel(one.table()[list(FLOAT_ROWS)], R[list(FLOAT_ROWS)]), "mcmc", dtype)
    # summary_only: the blocks never reach the host, the accumulator sees the same draws
    plain = la.mcmc(init, kern, summary_only=True, **kw)
    rk3 = la.RankDiagnostics(64, 8, 40, dtype)
    with_rk = la.mcmc(init, kern, summary_only=True, rank=rk3, **kw)
    assert set(with_rk) == set(plain) | {"rank"} and all(same(plain[k], with_rk[k]) for k in plain)
    assert same(with_rk["rank"], one.result()) and everything(rk3) == everything(one)
    assert np.array_equal(plain["state"], info["state"]) and with_rk["rank"]["n_used"] == 40 and with_rk["rank"]["chains"] == 64
    with pytest.raises(ValueError, match="holds 40"):
        la.mcmc(init, kern, summary_only=True, rank=rk3, **kw)  # no room for 40 more
    for q in (rk, one, rk3):
        q.free()
    model.close()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_with_a_reason(la):
    import ctypes as C
    from logreg_amd import _lib
    for kw, word in ((dict(max_lag=64), "odd"), (dict(max_lag=257), "odd"), (dict(max_lag=0), "odd"), (dict(dtype="int32"), "dtype")):
        with pytest.raises(ValueError, match=word):
            la.RankDiagnostics(5, 3, 8, **kw)
    for args in ((0, 3, 8), (5, 0, 8), (5, 3, 0)):
        with pytest.raises(ValueError, match="positive"):
            la.RankDiagnostics(*args)
    with pytest.raises(ValueError, match="beyond the cap"):
        la.RankDiagnostics(4097, 3, 4096)
    acc = la.RankDiagnostics(5, 3, 8, "float64")
    for bad in (np.zeros((2, 5, 4)), np.zeros((0, 5, 3)), np.zeros((5, 3))):
        with pytest.raises(ValueError):
            acc.update(bad)
    acc.update(np.zeros((8, 5, 3)))
    with pytest.raises(ValueError, match="exceed max_steps"):
        acc.update(np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match="coordinate"):
        acc.ranks(3)
    acc.free()
    L = _lib.load_rank()
    h = C.c_void_p()
    for args, word in (((0, 0, 5, 3, 8, 64), "odd"), ((0, 0, 5, 3, 8, 257), "odd"), ((0, 0, 0, 3, 8, 63), "positive"), ((0, 0, 5, 0, 8, 63), "positive"),
                       ((0, 0, 5, 3, 0, 63), "positive"), ((0, 7, 5, 3, 8, 63), "dtype"), ((0, 0, 4097, 3, 4096, 63), "LR_RANK_MAX_DRAWS"),
                       ((0, 0, 3, 3, 2**62, 63), "LR_RANK_MAX_DRAWS")):
        assert L.lr_rank_create(*args, C.byref(h)) != 0 and word in L.lr_last_error().decode(), args
    assert L.lr_rank_create(0, 0, 5, 3, 8, 63, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_rank_create(0, 1, 5, 3, 8, 63, C.byref(h)) == 0
    x = np.zeros((9, 5, 3))
    n = C.c_int64(-1)
    T = np.empty((15, 3))
    assert L.lr_rank_accumulate(h, None, 2, 0, None) != 0 and "NULL" in L.lr_last_error().decode()
    assert L.lr_rank_accumulate(None, x.ctypes.data, 2, 0, None) != 0
    assert L.lr_rank_accumulate(h, x.ctypes.data, 0, 0, None) != 0 and "positive" in L.lr_last_error().decode()
    assert L.lr_rank_accumulate(h, x.ctypes.data, 9, 0, None) != 0 and "exceed max_steps" in L.lr_last_error().decode()
    assert L.lr_rank_result(h, T.ctypes.data, C.byref(n)) == 0 and n.value == 0 and np.all(np.isnan(T[:11]))  # refused calls left it empty
    assert L.lr_rank_accumulate(h, x.ctypes.data, 8, 0, None) == 0 and L.lr_rank_accumulate(h, x.ctypes.data, 1, 0, None) != 0
    assert L.lr_rank_result(h, T.ctypes.data, C.byref(n)) == 0 and n.value == 8
    assert L.lr_rank_result(h, None, None) != 0 and L.lr_rank_reset(None) != 0 and L.lr_rank_ranks(h, 0, 0, None, None, None) != 0
    L.lr_rank_destroy(h)
    L.lr_rank_destroy(None)


def measure():
    """Print the largest error of z and of the statistics over every case (profiles/r28_rank.txt section 1)."""
    global _MEASURED
    import logreg_amd as la
    _MEASURED = {}
    for shape in cases.SHAPES:
        for dtype in cases.DTYPES:
            check_ranks(la, shape, dtype)
            check_statistics(la, shape, dtype)
    test_the_two_cases_the_classical_rhat_is_blind_to(la)
    for dtype in cases.DTYPES:
        test_fewer_than_four_steps_and_a_constant_column_give_nan(la, dtype)
        test_mcmc_feeds_the_accumulator_without_changing_the_run(la, dtype)
    for what, v in _MEASURED.items():
        print(f"FIGURE largest error {what} {v:.3e}   (bound in force: {BOUND[what]:.3e})")


if __name__ == "__main__":
    if sys.argv[1:] != ["--measure"]:
        sys.exit("usage: python tests/test_gpu_rank.py --measure")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
