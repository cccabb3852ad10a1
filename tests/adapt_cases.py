"""TEST INFRASTRUCTURE: the shapes of the warm-up tests (tests/test_gpu_adapt.py, tests/test_adapt_cpu.py) and the driver that runs a
warm-up through the C ABI of include/logreg_hip_adapt.h, in pieces, from host or device memory.

Model: synthetic, n = 50 rows, max_depth = 5.  Chains 1, 3, 65, 257, 1025 (1025: more than four partials and a ragged last workgroup);
p = 3, 8, 16, 20 (every padded width 4, 8, 16, 32); W = 19 (no window), 60 (proportional buffers), 150 (one exact window), 260 (two
windows, 75-100 and 100-210)."""
import ctypes as C

import numpy as np

N_ROWS = 50
MAX_DEPTH = 5
DTYPES = ("float32", "float64")
CHAINS = (1, 3, 65, 257, 1025)
WIDTHS = (3, 8, 16, 20)
WARMUPS = (19, 60, 150, 260)
# (C, p, W): the whole product of the three sets, 80 shapes (each a fraction of a second)
CASES = [(c, p, w) for c in CHAINS for p in WIDTHS for w in WARMUPS]
# Relative tolerance of the teacher-forced step-size comparison: 8 x the largest deviation measured on the MI355X over CASES x DTYPES
# (profiles/r18_adapt.txt).  The deviation is the device library's exp / log / pow against NumPy's and one ulp of abar_t, carried through
# the recursion.
EPS_RTOL_MEASURED = 9.340e-15  # float64, C = 1025, p = 8, W = 260
EPS_RTOL = 8 * EPS_RTOL_MEASURED
# the hand-listed window ends of the issue: W -> (init, ends)
HAND_SCHEDULE = {1000: (75, [100, 150, 250, 450, 950]), 150: (75, [100]), 60: (9, [54]), 260: (75, [100, 210]), 19: (19, [])}


def case_id(c):
    return "C%d_p%d_W%d" % c


def data(p):
    from logreg_amd import synthetic_logreg
    X, y, _ = synthetic_logreg(N_ROWS, p, seed=20260000 + p)
    return X, y, np.ones(p)


def start(Cn, p, seed=11):
    return 0.3 * np.random.default_rng(seed + 1000 * p + Cn).standard_normal((Cn, p))


def warm(model, q0, W, *, seed=5, chain_offset=0, cuts=None, on_device=False, dmm0=None, adapt_metric=True, eps0=0.0, max_depth=MAX_DEPTH, L=None,
         want=("out", "depth", "astat")):
    """One warm-up of `model` from q0 [C, p] through lr_adapt_*: `cuts` = the iterations of each lr_adapt_run call (default: one call).
    -> dict(state, out [W,C,p], depth [W,C], astat [W,C], counters, eps, dmm, info, trace [W,5], metric [windows,2,p])"""
    from logreg_amd import DeviceArray, _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_adapt(model._L if L is None else L)
    Cn, p = q0.shape
    dt = model.np_dtype
    st = np.array(q0, dtype=dt, order="C")
    d0 = None if dmm0 is None else np.ascontiguousarray(dmm0, dtype=np.float64)
    o = _lib.AdaptOpts(W=W, adapt_metric=int(adapt_metric), eps0=eps0, dmm0=None if d0 is None else d0.ctypes.data)
    h = C.c_void_p()
    _lib.check(L.lr_adapt_create(model.handle, Cn, C.byref(o), C.byref(h)))
    try:
        out = np.zeros((W, Cn, p), dtype=dt)
        depth = np.zeros((W, Cn), dtype=np.int8)
        astat = np.zeros((W, Cn), dtype=np.float64)
        counters = np.zeros(Cn, dtype=NUTS_COUNTERS)
        host = {"state": st, "out": out, "depth": depth, "astat": astat, "counters": counters}
        dev = {k: DeviceArray.from_host(model.device, v) for k, v in host.items()} if on_device else None
        opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, seed=seed, group=0, mode=_lib.MODE_AUTO, on_device=int(on_device))
        t = 0
        for k in (cuts or [W]):
            def ptr(name, per_iter):
                if name != "state" and name != "counters" and name not in want:
                    return None
                if on_device:
                    return dev[name].ptr + t * per_iter
                return host[name].ctypes.data + t * per_iter
            _lib.check(L.lr_adapt_run(h, ptr("state", 0), k, max_depth, C.byref(opts), ptr("out", Cn * p * st.itemsize), ptr("counters", 0),
                                      ptr("depth", Cn), ptr("astat", Cn * 8)))
            t += k
        e, info = C.c_double(), _lib.AdaptInfo()
        dmm = np.empty(p)
        _lib.check(L.lr_adapt_result(h, C.byref(e), dmm.ctypes.data, C.byref(info)))
        trace = np.zeros((W, _lib.ADAPT_TRACE_COLS))
        metric = np.zeros((info.n_windows, 2, p))
        _lib.check(L.lr_adapt_trace(h, trace.ctypes.data, metric.ctypes.data if info.n_windows else None))
        if on_device:
            _lib.check(L.lr_stream_sync(model.device, None))
            host = {k: v.to_host() for k, v in dev.items()}
            for v in dev.values():
                v.free()
    finally:
        L.lr_adapt_destroy(h)
    return {"state": host["state"], "out": host["out"], "depth": host["depth"], "astat": host["astat"], "counters": host["counters"], "eps": e.value, "dmm": dmm,
            "info": {"iterations": info.iterations, "metric_skipped": info.metric_skipped, "windows": info.windows, "n_windows": info.n_windows},
            "trace": trace, "metric": metric}


def same_bytes(a, b, keys=("state", "out", "depth", "astat", "trace", "metric", "dmm")):
    """the first key whose bytes differ between two results of warm(), or None"""
    for k in keys:
        if a[k].tobytes() != b[k].tobytes():
            return k
    if np.float64(a["eps"]).tobytes() != np.float64(b["eps"]).tobytes() or a["info"] != b["info"] or a["counters"].tobytes() != b["counters"].tobytes():
        return "result"
    return None
