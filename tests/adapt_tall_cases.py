"""TEST INFRASTRUCTURE: the shapes of the tests of the NUTS warm-up on the stepwise engine (tests/test_gpu_adapt_tall.py,
tests/test_adapt_tall_cpu.py), the driver that runs one through the C ABI of include/logreg_hip_adapt_tall.h, and the NumPy restatement
of the header's workgroup order at the wide lane maps (Q = 4 and 2).

Models: nuts_reference.synthetic_model.  Narrow p = 3, 8, 17, 32 at the row counts of nuts_tall_cases.N_F64 / N_F32 (601 .. 9001: the
fewest the stepwise mode accepts for NUTS), wide p = 33, 64, 65, 128 (P = 64: a chain fills one wave; P = 128: two) at n = 100.  Chains
1, 3, 65, 257 (257 at P = 128: the second workgroup of k_tall_adapt_partial holds one chain).  W = 19 (no window), 40 (proportional
buffers: one window, 6 .. 36), 150 (the exact buffers: one window, 75 .. 100); max_depth 5."""
import ctypes as C

import numpy as np

import adapt_cases
import nuts_reference as nr
import nuts_tall_cases as ntc

MAX_DEPTH = 5
DTYPES = ("float32", "float64")
NARROW = (3, 8, 17, 32)
WIDE = (33, 64, 65, 128)
CHAINS = (1, 3, 65, 257)
# (p, C, W): every padded width with every chain count once, every W at both kinds of width
REPLAY = [(3, 3, 40), (8, 65, 150), (17, 1, 40), (32, 257, 19), (33, 65, 40), (64, 1, 19), (65, 3, 150), (128, 257, 40)]
TEACHER = [(3, 257, 40), (8, 1, 150), (17, 65, 40), (32, 3, 150), (33, 3, 150), (64, 257, 40), (65, 65, 19), (128, 1, 40), (128, 257, 150)]
# Relative tolerance of the teacher-forced step-size comparison: max(the fused warm-up's, 8 x the largest deviation measured on the MI355X
# over TEACHER x DTYPES) -- profiles/r26_adapt_tall.txt.  The arithmetic of the update kernel's lane 0 is the fused warm-up's, so is the
# deviation: the device library's exp / log / pow against NumPy's and one ulp of abar_t, carried through the recursion.
EPS_RTOL_MEASURED = 4.451e-15  # float32, p = 64, C = 257, W = 40
EPS_RTOL = max(adapt_cases.EPS_RTOL, 8 * EPS_RTOL_MEASURED)


def case_id(c):
    return "p%d_C%d_W%d" % c


def rows(p, dtype):
    return 100 if p > 32 else (ntc.N_F32 if dtype == "float32" else ntc.N_F64)[p]


def data(p, dtype):
    """-> X, y, pscale of the model of width p in `dtype`"""
    return nr.synthetic_model(p, rows(p, dtype), 100 + p)


def start(Cn, p, n, seed=11):
    """starts at the posterior's scale, ~ 1 / sqrt(n) around 0"""
    return 2.0 * n ** -0.5 * np.random.default_rng(seed + 1000 * p + Cn).standard_normal((Cn, p))


def warm(model, q0, W, *, seed=5, chain_offset=0, cuts=None, on_device=False, dmm0=None, adapt_metric=True, eps0=0.0, max_depth=MAX_DEPTH, group=0, L=None):
    """adapt_cases.warm through lr_tall_adapt_create / lr_tall_adapt_run (mode = stepwise, `group` slices asked); the same result dict"""
    from logreg_amd import DeviceArray, _lib
    from logreg_amd.kernels import NUTS_COUNTERS
    L = _lib.bind_adapt_tall(model._L if L is None else L)
    Cn, p = q0.shape
    st = np.array(q0, dtype=model.np_dtype, order="C")
    d0 = None if dmm0 is None else np.ascontiguousarray(dmm0, dtype=np.float64)
    o = _lib.AdaptOpts(W=W, adapt_metric=int(adapt_metric), eps0=eps0, dmm0=None if d0 is None else d0.ctypes.data)
    h = C.c_void_p()
    _lib.check(L.lr_tall_adapt_create(model.handle, Cn, C.byref(o), C.byref(h)))
    try:
        host = {"state": st, "out": np.zeros((W, Cn, p), dtype=st.dtype), "depth": np.zeros((W, Cn), dtype=np.int8), "astat": np.zeros((W, Cn)),
                "counters": np.zeros(Cn, dtype=NUTS_COUNTERS)}
        per_iter = {"state": 0, "out": Cn * p * st.itemsize, "depth": Cn, "astat": Cn * 8, "counters": 0}
        dev = {k: DeviceArray.from_host(model.device, v) for k, v in host.items()} if on_device else None
        opts = _lib.RunOpts(n_chains=Cn, chain_offset=chain_offset, thin=1, iters=1, seed=seed, group=group, mode=_lib.MODE_STEPWISE, on_device=int(on_device))
        t = 0
        for k in (cuts or [W]):
            at = {name: (dev[name].ptr if on_device else host[name].ctypes.data) + t * per_iter[name] for name in host}
            _lib.check(L.lr_tall_adapt_run(h, at["state"], k, max_depth, C.byref(opts), at["out"], at["counters"], at["depth"], at["astat"]))
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
    return dict(host, eps=e.value, dmm=dmm, trace=trace, metric=metric,
                info={"iterations": info.iterations, "metric_skipped": info.metric_skipped, "windows": info.windows, "n_windows": info.n_windows})


same_bytes = adapt_cases.same_bytes


def step_size_deviation(res, tf):
    """the largest relative deviation of the eps sequence, log_eps_bar and the final eps of a warm-up from the teacher-forced reference"""
    tr = res["trace"]
    return max(np.max(np.abs(tr[:, 0] - tf["eps"]) / tf["eps"]), np.max(np.abs(tr[:, 2] - tf["log_eps_bar"]) / np.maximum(np.abs(tf["log_eps_bar"]), 1.0)),
               abs(res["eps"] - tf["final"]) / tf["final"])


# ---- include/logreg_hip_adapt_tall.h's workgroup order in NumPy float64, one operation per operator as the header writes them
def padded(p):
    return next(P for P in (4, 8, 16, 32, 64, 128) if p <= P)


def _fma(a, b, c):
    """fma(a, b, c) rounded once: the product and the sum in np.longdouble (64-bit significand: the product of two float64 numbers is exact
    to 2^-64 relative, below half an ulp of the rounded sum by 2^-11 -- a double rounding can show only on a tie, and the bounds of
    adapt_reference.py are far wider than one ulp)"""
    L = np.longdouble
    return (np.asarray(a, dtype=L) * np.asarray(b, dtype=L) + np.asarray(c, dtype=L)).astype(np.float64)


def _merge(na, ma, Ma, nb, mb, Mb):
    n, d = na + nb, mb - ma
    return n, _fma(d, nb / n, ma), _fma(d * d, na * nb / n, Ma + Mb)


def sum256(v):
    s = np.zeros(256)
    s[:len(v)] = v
    h = 128
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def header_order(astat, draws, W, dmm0, adapt_metric=True):
    """The header's arithmetic in its order: -> dict(abar [W], metric [(var, dmm, skipped) per window], dmm, skipped).  draws [W, C, p]."""
    import adapt_reference as ar
    astat, draws = np.asarray(astat, dtype=np.float64), np.asarray(draws).astype(np.float64)
    Cn, p = draws.shape[1:]
    Q = 256 // padded(p)
    init, ends = ar.schedule(W) if adapt_metric else (W, [])
    idx, lasts = ar.windows_of(W, init, ends)
    abar = np.empty(W)
    dmm = np.array(np.broadcast_to(np.asarray(dmm0, dtype=np.float64), (p,)))
    win, metric, skipped = None, [], 0
    for t in range(W):
        tot = np.float64(0.0)
        for k, b in enumerate(range(0, Cn, 256)):
            part = sum256(astat[t, b:b + 256])
            tot = part if k == 0 else tot + part
        abar[t] = tot / np.float64(Cn)
        if idx[t] < 0:
            continue
        it = None
        for b in range(0, Cn, 256):
            x = draws[t, b:b + 256]
            nb = np.float64(len(x))
            s = np.zeros((Q, p))
            for i in range(len(x)):
                s[i % Q] = s[i % Q] + x[i]
            h = Q // 2
            while h:
                s[:h] = s[:h] + s[h:2 * h]
                h //= 2
            mean = s[0] / nb
            e = np.zeros((Q, p))
            for i in range(len(x)):
                d = x[i] - mean
                e[i % Q] = _fma(d, d, e[i % Q])
            h = Q // 2
            while h:
                e[:h] = e[:h] + e[h:2 * h]
                h //= 2
            it = (nb, mean, e[0].copy()) if it is None else _merge(*it, nb, mean, e[0])
        win = it if win is None else _merge(*win, *it)
        if t in lasts:
            n = win[0]
            with np.errstate(all="ignore"):
                var = win[2] / (n - 1.0)
                ok = (var > 0) & (var < np.inf)
                inv = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0))
                dmm = np.where(ok, 1.0 / np.where(ok, inv, 1.0), dmm)
            metric.append((var, dmm.copy(), ~ok))
            skipped += int((~ok).sum())
            win = None
    return {"abar": abar, "metric": metric, "dmm": dmm, "skipped": skipped}
