"""The two ways into a run give the same bytes: host pointers (on_device = 0: the library stages every array through device buffers
of its own, launches on the NULL stream and copies back) and device buffers on a stream (on_device = 1).

Through the C ABI itself, on the Pima model in both dtypes, for rwmh, mala, ul, hmc and nuts: C = 3 chains (a count that fills no lane
group), iters = 2, thin = 2, a statistics window.  state, out, accepts (nuts: the counters and depth_out), lp_state (rwmh, mala) and
the statistics buffer must agree byte for byte, and again with out, accepts / counters and depth_out left out (NULL).  accepts and
counters start from non-zero values: launches add to them, so they travel in as well as out.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAINS, ITERS, THIN, P = 3, 2, 2, 8
PRE = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])
KINDS = ("rwmh", "mala", "ul", "hmc", "nuts")


@pytest.fixture(autouse=True)
def step_timeout():
    """Every test under its own time limit: one that hangs ends the whole run (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def models(pima, pscale):
    import logreg_amd as la
    X, y = pima
    return {dt: la.LogReg(X, y, pscale, dtype=dt, device=0) for dt in ("float32", "float64")}


def arrays(kind, np_dtype, map_beta, optional):
    """name -> host array of one call, in the order they are compared; `optional` False leaves out what the ABI lets a caller leave out"""
    from logreg_amd import _lib
    sd = np.array([1.71, 0.0655, 0.0068, 0.0184, 0.0226, 0.0429, 0.547, 0.0225])
    a = {"state": (map_beta + 0.5 * sd * np.random.default_rng(3).standard_normal((CHAINS, P))).astype(np_dtype)}
    if kind in ("rwmh", "mala"):
        a["lp_state"] = np.full(CHAINS, -np.inf)  # (-inf: the kernel evaluates the state it was given)
    a["stats"] = np.zeros((2, CHAINS, 2, P))
    if optional:
        a["out"] = np.zeros((ITERS, CHAINS, P), np_dtype)
        if kind == "nuts":
            a["tally"] = np.zeros(CHAINS, np.dtype(_lib.NutsCounters))
            a["tally"]["n_leapfrog"] = 5
            a["depth_out"] = np.zeros((ITERS, CHAINS), np.int8)
        else:
            a["tally"] = np.arange(7, 7 + CHAINS, dtype=np.uint32)
    return a


def call(L, model, kind, ptr, on_device, stream):
    from logreg_amd import _lib
    o = _lib.RunOpts(n_chains=CHAINS, thin=THIN, iters=ITERS, seed=0x5EED, mode=_lib.MODE_AUTO, on_device=on_device, stream=stream,
                     stats=ptr("stats"), stats_batch=1, stats_first=0, stats_slots=2)
    h, vec = model.handle, np.ascontiguousarray(1.0 / PRE)
    if kind == "rwmh":
        sd = np.ascontiguousarray(0.1 / np.sqrt(PRE))
        return L.lr_run_rwmh(h, ptr("state"), ptr("lp_state"), sd.ctypes.data, C.byref(o), ptr("out"), ptr("tally"))
    if kind == "mala":
        return L.lr_run_mala(h, ptr("state"), ptr("lp_state"), 1e-4, vec.ctypes.data, C.byref(o), ptr("out"), ptr("tally"))
    if kind == "ul":
        return L.lr_run_ul(h, ptr("state"), 1e-4, vec.ctypes.data, C.byref(o), ptr("out"), ptr("tally"))
    if kind == "hmc":
        return L.lr_run_hmc(h, ptr("state"), 1e-3, 5, vec.ctypes.data, C.byref(o), ptr("out"), ptr("tally"))
    return L.lr_run_nuts(h, ptr("state"), 1e-3, 4, vec.ctypes.data, C.byref(o), ptr("out"), ptr("tally"), ptr("depth_out"))


def through_host_pointers(L, model, kind, a):
    from logreg_amd import _lib
    _lib.check(call(L, model, kind, lambda k: a[k].ctypes.data if k in a else None, 0, None))
    return a


def through_device_buffers(L, model, kind, a):
    from logreg_amd import _lib
    stream, dev = C.c_void_p(), {}
    _lib.check(L.lr_stream_create(0, C.byref(stream)))
    try:
        for k, v in a.items():
            dev[k] = C.c_void_p()
            _lib.check(L.lr_malloc(0, v.nbytes, C.byref(dev[k])))
            _lib.check(L.lr_memcpy_h2d(0, dev[k], v.ctypes.data, v.nbytes, stream))
        _lib.check(call(L, model, kind, lambda k: dev[k].value if k in dev else None, 1, stream))
        for k, v in a.items():
            _lib.check(L.lr_memcpy_d2h(0, v.ctypes.data, dev[k], v.nbytes, stream))
        _lib.check(L.lr_stream_sync(0, stream))
    finally:
        for d in dev.values():
            if d.value:
                L.lr_free(0, d)
        L.lr_stream_destroy(0, stream)
    return a


@pytest.mark.parametrize("optional", [True, False], ids=["every-array", "optional-arrays-left-out"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_host_pointers_and_device_buffers_give_the_same_bytes(models, map_beta, dtype, kind, optional):
    from logreg_amd import _lib
    L = _lib.load_nuts()
    np_dtype = np.float32 if dtype == "float32" else np.float64
    start = arrays(kind, np_dtype, map_beta, optional)
    host = through_host_pointers(L, models[dtype], kind, arrays(kind, np_dtype, map_beta, optional))
    dev = through_device_buffers(L, models[dtype], kind, arrays(kind, np_dtype, map_beta, optional))
    assert list(host) == list(dev)
    for k in host:
        assert host[k].tobytes() == dev[k].tobytes(), (dtype, kind, k, host[k], dev[k])
    # ... and the run did run: the state moved or was weighed, the statistics window was written, the tallies were added to
    assert np.all(np.isfinite(host["state"])) and host["stats"].tobytes() != start["stats"].tobytes()
    if "lp_state" in host:
        assert np.all(np.isfinite(host["lp_state"]))
    if optional:
        assert np.array_equal(host["out"][-1], host["state"])
        if kind == "nuts":
            assert np.all(host["tally"]["n_leapfrog"] > 5) and np.all(host["depth_out"] != 0)
        else:
            assert np.all(host["tally"] >= start["tally"]) and np.all(host["tally"] <= start["tally"] + ITERS * THIN)
