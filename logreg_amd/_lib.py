"""ctypes binding of liblogreg_hip.so (the C ABI in include/logreg_hip.h).

There is no CPU fallback: if the library cannot be loaded, or no MI355X is visible, every entry
point raises.  Nothing in this package imports the test oracle under oracle/.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "liblogreg_hip.so")

LR_F32, LR_F64 = 0, 1
STATS_ROWS = 7  # LR_STATS_ROWS
PREC_BY_NAME = {"auto": 0, "full": 1, "bf16": 2}  # LR_PREC_*
KIND_BY_NAME = {"rwmh": 0, "mala": 1, "hmc": 2, "ul": 3, "nuts": 4, "pg": 6}  # LR_KIND_* (LR_KIND_NUTS: include/logreg_hip_nuts.h, LR_KIND_PG: logreg_hip_pg.h)
NUTS_MAX_DEPTH = 10  # LR_NUTS_MAX_DEPTH
MODE_AUTO, MODE_REG, MODE_LDS, MODE_GLOBAL, MODE_MFMA, MODE_STEPWISE, MODE_MIXED = -1, 0, 1, 2, 3, 4, 5
MODE_NAMES = {MODE_REG: "reg", MODE_LDS: "lds", MODE_GLOBAL: "global", MODE_MFMA: "mfma", MODE_STEPWISE: "stepwise", MODE_MIXED: "mixed"}
MODE_BY_NAME = {"auto": MODE_AUTO, "reg": MODE_REG, "lds": MODE_LDS, "global": MODE_GLOBAL, "mfma": MODE_MFMA, "stepwise": MODE_STEPWISE, "mixed": MODE_MIXED}


class LogregHipError(RuntimeError):
    pass


class RunOpts(C.Structure):
    _fields_ = [("n_chains", C.c_int64), ("chain_offset", C.c_int64), ("thin", C.c_int64), ("iters", C.c_int64),
                ("iter_offset", C.c_int64), ("seed", C.c_uint64), ("group", C.c_int32), ("mode", C.c_int32),
                ("on_device", C.c_int32), ("stream", C.c_void_p),
                ("stats", C.c_void_p), ("stats_batch", C.c_int64), ("stats_first", C.c_int64), ("stats_slots", C.c_int64),
                ("precision", C.c_int32), ("plan_chains", C.c_int32), ("plan_first", C.c_int64)]


class PlanInfo(C.Structure):
    _fields_ = [("mode", C.c_int32), ("group", C.c_int32), ("rows", C.c_int32), ("tail_group", C.c_int32), ("tail_rows", C.c_int32),
                ("split", C.c_int64), ("tail_mode", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); every symbol include/logreg_hip.h declares
_vp, _dp, _i32, _i64, _u64 = C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int64, C.c_uint64
_op = C.POINTER(RunOpts)
SYMBOLS = {
    "lr_last_error": (C.c_char_p, []),
    "lr_build_id": (C.c_char_p, []),
    "lr_sizeof_run_opts": (C.c_int, []),
    "lr_device_count": (C.c_int, []),
    "lr_device_cus": (C.c_int, [C.c_int]),
    "lr_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "lr_model_create": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, C.POINTER(_vp)]),
    "lr_model_destroy": (None, [_vp]),
    "lr_model_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "lr_model_debug_opts": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "lr_model_interior_format": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "lr_eval": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _op]),
    "lr_run_rwmh": (C.c_int, [_vp, _vp, _vp, _vp, _op, _vp, _vp]),
    "lr_run_mala": (C.c_int, [_vp, _vp, _vp, C.c_double, _vp, _op, _vp, _vp]),
    "lr_run_ul": (C.c_int, [_vp, _vp, C.c_double, _vp, _op, _vp, _vp]),
    "lr_run_hmc": (C.c_int, [_vp, _vp, C.c_double, _i32, _vp, _op, _vp, _vp]),
    "lr_hessian": (C.c_int, [_vp, _vp, _dp, _vp, _vp, _vp]),
    "lr_stats_reduce": (C.c_int, [C.c_int, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp]),
    "lr_plan_run": (C.c_int, [_vp, _i32, _op, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "lr_plan_run_info": (C.c_int, [_vp, _i32, _op, C.c_void_p]),
    "lr_plan": (C.c_int, [_vp, _i64, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "lr_malloc": (C.c_int, [C.c_int, _u64, C.POINTER(_vp)]),
    "lr_free": (C.c_int, [C.c_int, _vp]),
    "lr_memcpy_h2d": (C.c_int, [C.c_int, _vp, _vp, _u64, _vp]),
    "lr_memcpy_d2h": (C.c_int, [C.c_int, _vp, _vp, _u64, _vp]),
    "lr_memset": (C.c_int, [C.c_int, _vp, C.c_int, _u64, _vp]),
    "lr_stream_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "lr_stream_destroy": (C.c_int, [C.c_int, _vp]),
    "lr_stream_sync": (C.c_int, [C.c_int, _vp]),
    "lr_event_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "lr_event_destroy": (C.c_int, [C.c_int, _vp]),
    "lr_event_record": (C.c_int, [C.c_int, _vp, _vp]),
    "lr_event_elapsed_ms": (C.c_int, [C.c_int, _vp, _vp, C.POINTER(C.c_float)]),
    # the C-level exchange (RCCL, loaded at first use); the Python face itself goes through torch.distributed
    "lr_comm_unique_id": (C.c_int, [_vp]),
    "lr_comm_create": (C.c_int, [_vp, _i32, _i32, C.c_int, C.POINTER(_vp)]),
    "lr_comm_destroy": (C.c_int, [_vp]),
    "lr_gather": (C.c_int, [_vp, _vp, _vp, _u64, _i32, _vp]),
    "lr_allreduce_sum_f64": (C.c_int, [_vp, _vp, _u64, _vp]),
}


class NutsCounters(C.Structure):  # lr_nuts_counters (include/logreg_hip_nuts.h)
    _fields_ = [("n_leapfrog", C.c_uint64), ("depth_sum", C.c_uint64), ("accept_stat_sum", C.c_double), ("divergent", C.c_uint32),
                ("max_depth_hits", C.c_uint32)]


# name -> (restype, argtypes); every symbol include/logreg_hip_nuts.h declares.  A table of its own, bound on first use (load_nuts):
# SYMBOLS is the exact symbol set of logreg_hip.h
NUTS_SYMBOLS = {
    "lr_run_nuts": (C.c_int, [_vp, _vp, C.c_double, _i32, _vp, _op, _vp, _vp, _vp]),
}

PRED_ROWS = 5  # LR_PRED_ROWS
# name -> (restype, argtypes); every symbol include/logreg_hip_predict.h declares.  A table of its own like NUTS_SYMBOLS, bound on
# first use (load_predict): the test doubles bind SYMBOLS / NUTS_SYMBOLS onto libraries that do not have these
PREDICT_SYMBOLS = {
    "lr_predict_create": (C.c_int, [_vp, _vp, _vp, _i64, C.POINTER(_vp)]),
    "lr_predict_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_predict_result": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "lr_predict_reset": (C.c_int, [_vp]),
    "lr_predict_destroy": (None, [_vp]),
}

ACF_MAX_LAG = 255  # LR_ACF_MAX_LAG
ACF_HEAD_ROWS = 3  # rows of the table ahead of the autocovariances: LR_ACF_ROWS(K) = K + 4
# name -> (restype, argtypes); every symbol include/logreg_hip_acf.h declares.  A table of its own like PREDICT_SYMBOLS, bound on first
# use (load_acf)
ACF_SYMBOLS = {
    "lr_acf_create": (C.c_int, [C.c_int, _i32, _i64, _i32, _i32, C.POINTER(_vp)]),
    "lr_acf_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_acf_result": (C.c_int, [_vp, _vp, _vp, C.POINTER(_i64)]),
    "lr_acf_reset": (C.c_int, [_vp]),
    "lr_acf_destroy": (None, [_vp]),
}

MARG_MAX_BINS = 1024  # LR_MARG_MAX_BINS
MARG_ROWS = 6  # LR_MARG_ROWS: min, max, S1..S4; a coordinate has LR_MARG_COLS(B) = B + 3 columns (underflow, B bins, overflow, NaN)
# name -> (restype, argtypes); every symbol include/logreg_hip_marginals.h declares.  A table of its own like ACF_SYMBOLS, bound on first
# use (load_marginals)
MARG_SYMBOLS = {
    "lr_marg_create": (C.c_int, [C.c_int, _i32, _i64, _i32, _i32, _vp, _vp, C.POINTER(_vp)]),
    "lr_marg_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_marg_result": (C.c_int, [_vp, _vp, _vp, C.POINTER(_i64)]),
    "lr_marg_reset": (C.c_int, [_vp]),
    "lr_marg_destroy": (None, [_vp]),
}

LOO_ROWS = 5  # LR_LOO_ROWS: elpd_loo_i, khat_i, n_eff_i, lppd_i, n_tail_i
LOO_MAX_DRAWS = 1 << 20  # LR_LOO_MAX_DRAWS
# name -> (restype, argtypes); every symbol include/logreg_hip_loo.h declares.  A table of its own like MARG_SYMBOLS, bound on first
# use (load_loo)
LOO_SYMBOLS = {
    "lr_loo_create": (C.c_int, [_vp, _i64, C.POINTER(_vp)]),
    "lr_loo_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_loo_loglik": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "lr_loo_result": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "lr_loo_reset": (C.c_int, [_vp]),
    "lr_loo_destroy": (None, [_vp]),
    "lr_psis": (C.c_int, [C.c_int, _vp, _i64, _i64, _i32, _i32, _vp, _vp]),
}

COV_MAX_P = 128  # LR_COV_MAX_P
# name -> (restype, argtypes); every symbol include/logreg_hip_cov.h declares.  A table of its own like MARG_SYMBOLS, bound on first use
# (load_covariance)
COV_SYMBOLS = {
    "lr_cov_create": (C.c_int, [C.c_int, _i32, _i64, _i32, _vp, _vp, C.POINTER(_vp)]),
    "lr_cov_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_cov_result": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "lr_cov_reset": (C.c_int, [_vp]),
    "lr_cov_destroy": (None, [_vp]),
}

ADAPT_ITER_BASE = 1 << 62  # LR_ADAPT_ITER_BASE
ADAPT_MAX_WINDOWS = 32  # LR_ADAPT_MAX_WINDOWS
ADAPT_TRACE_COLS = 5  # LR_ADAPT_TRACE_COLS


class AdaptOpts(C.Structure):  # lr_adapt_opts (include/logreg_hip_adapt.h)
    _fields_ = [("W", C.c_int32), ("adapt_metric", C.c_int32), ("delta", C.c_double), ("eps0", C.c_double), ("dmm0", C.c_void_p),
                ("gamma", C.c_double), ("t0", C.c_double), ("kappa", C.c_double), ("init_buffer", C.c_int32), ("term_buffer", C.c_int32),
                ("base_window", C.c_int32), ("reserved", C.c_int32)]


class AdaptInfo(C.Structure):  # lr_adapt_info
    _fields_ = [("iterations", C.c_int64), ("metric_skipped", C.c_int64), ("windows", C.c_int32), ("n_windows", C.c_int32)]


# name -> (restype, argtypes); every symbol include/logreg_hip_adapt.h declares.  A table of its own like COV_SYMBOLS, bound on first use
# (load_adapt)
ADAPT_SYMBOLS = {
    "lr_adapt_schedule": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "lr_adapt_create": (C.c_int, [_vp, _i64, C.POINTER(AdaptOpts), C.POINTER(_vp)]),
    "lr_adapt_run": (C.c_int, [_vp, _vp, _i64, _i32, _op, _vp, _vp, _vp, _vp]),
    "lr_adapt_result": (C.c_int, [_vp, _dp, _vp, C.POINTER(AdaptInfo)]),
    "lr_adapt_trace": (C.c_int, [_vp, _vp, _vp]),
    "lr_adapt_destroy": (None, [_vp]),
}

# name -> (restype, argtypes); every symbol include/logreg_hip_adapt_tall.h declares: the warm-up on the stepwise engine.  A table of its
# own like ADAPT_SYMBOLS, bound on first use (load_adapt_tall); the handle is an lr_adapt, read and destroyed through ADAPT_SYMBOLS
ADAPT_TALL_SYMBOLS = {
    "lr_tall_adapt_create": ADAPT_SYMBOLS["lr_adapt_create"],
    "lr_tall_adapt_run": ADAPT_SYMBOLS["lr_adapt_run"],
}

# name -> (restype, argtypes); every symbol include/logreg_hip_dense.h declares.  A table of its own like ADAPT_SYMBOLS, bound on first use
# (load_dense)
DENSE_SYMBOLS = {
    "lr_dense_factor": (C.c_int, [_i32, _vp, _vp, _vp, _vp]),
    "lr_run_nuts_dense": (C.c_int, [_vp, _vp, C.c_double, _i32, _vp, _op, _vp, _vp, _vp]),
    "lr_dense_adapt_create": (C.c_int, [_vp, _i64, C.POINTER(AdaptOpts), _vp, C.POINTER(_vp)]),
    "lr_dense_adapt_run": (C.c_int, [_vp, _vp, _i64, _i32, _op, _vp, _vp, _vp, _vp]),
    "lr_dense_adapt_result": (C.c_int, [_vp, _dp, _vp, C.POINTER(AdaptInfo)]),
    "lr_dense_adapt_trace": (C.c_int, [_vp, _vp, _vp]),
    "lr_dense_adapt_destroy": (None, [_vp]),
}

class PgCounters(C.Structure):  # lr_pg_counters (include/logreg_hip_pg.h)
    _fields_ = [("proposals", C.c_uint64), ("series_terms", C.c_uint64), ("skipped", C.c_uint32), ("reserved", C.c_uint32)]


PG_TAG = 0x10000000  # LR_PG_TAG
PG_MAX_ROWS = 65536  # LR_PG_MAX_ROWS
# name -> (restype, argtypes); every symbol include/logreg_hip_pg.h declares.  A table of its own like DENSE_SYMBOLS, bound on first use
# (load_pg)
PG_SYMBOLS = {
    "lr_run_pg": (C.c_int, [_vp, _vp, _op, _vp, _vp]),
    "lr_pg_omega": (C.c_int, [_vp, _vp, _op, _vp]),
}

class HsPrior(C.Structure):  # lr_hs_prior (include/logreg_hip_hs.h)
    _fields_ = [("shrink", C.c_void_p), ("global_scale", C.c_double)]


class HsCounters(C.Structure):  # lr_hs_counters
    _fields_ = [("proposals", C.c_uint64), ("series_terms", C.c_uint64), ("skipped", C.c_uint32), ("clamped", C.c_uint32)]


HS_TAG = 0x02000000  # LR_HS_TAG
HS_MIN, HS_MAX = 1e-100, 1e100  # LR_HS_MIN, LR_HS_MAX
# name -> (restype, argtypes); every symbol include/logreg_hip_hs.h declares.  A table of its own like PG_SYMBOLS, bound on first use
# (load_hs)
HS_SYMBOLS = {
    "lr_run_hs": (C.c_int, [_vp, C.POINTER(HsPrior), _vp, _vp, _op, _vp, _vp, _vp]),
    "lr_hs_hyper": (C.c_int, [_vp, C.POINTER(HsPrior), _vp, _vp, _op, _vp, _vp]),
}

BRIDGE_ROWS = 12  # LR_BRIDGE_ROWS: logml, se, iterations, converged, N1, N2, n_eff used, non-finite terms, min / max of l1 and of l2
BRIDGE_MAX_DRAWS = 1 << 20  # LR_BRIDGE_MAX_DRAWS
BRIDGE_TAG = 0x08000000  # LR_BRIDGE_TAG
# name -> (restype, argtypes); every symbol include/logreg_hip_bridge.h declares.  A table of its own like LOO_SYMBOLS, bound on first
# use (load_bridge)
BRIDGE_SYMBOLS = {
    "lr_bridge_create": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _u64, C.POINTER(_vp)]),
    "lr_bridge_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_bridge_terms": (C.c_int, [_vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "lr_bridge_proposal": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "lr_bridge_result": (C.c_int, [_vp, C.c_double, C.c_double, _i32, _vp]),
    "lr_bridge_reset": (C.c_int, [_vp]),
    "lr_bridge_destroy": (None, [_vp]),
    "lr_bridge_solve": (C.c_int, [C.c_int, _vp, _i64, _vp, _i64, C.c_double, C.c_double, _i32, _i32, _vp, _vp]),
}

RANK_MAX_LAG = 255  # LR_RANK_MAX_LAG
RANK_MAX_DRAWS = 1 << 24  # LR_RANK_MAX_DRAWS: draws per coordinate, chains x max_steps
RANK_ROWS = 15  # LR_RANK_ROWS
# name -> (restype, argtypes); every symbol include/logreg_hip_rank.h declares.  A table of its own like ACF_SYMBOLS, bound on first use
# (load_rank)
RANK_SYMBOLS = {
    "lr_rank_create": (C.c_int, [C.c_int, _i32, _i64, _i32, _i64, _i32, C.POINTER(_vp)]),
    "lr_rank_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_rank_result": (C.c_int, [_vp, _vp, C.POINTER(_i64)]),
    "lr_rank_ranks": (C.c_int, [_vp, _i32, _i32, _vp, _vp, C.POINTER(_i64)]),
    "lr_rank_reset": (C.c_int, [_vp]),
    "lr_rank_destroy": (None, [_vp]),
}

PPC_MAX_GROUPS = 32  # LR_PPC_MAX_GROUPS
PPC_TAG = 0x04000000  # LR_PPC_TAG
PPC_MOMENTS = 4  # LR_PPC_MOMENTS
# name -> (restype, argtypes); every symbol include/logreg_hip_ppc.h declares.  A table of its own like PREDICT_SYMBOLS, bound on first
# use (load_ppc)
PPC_SYMBOLS = {
    "lr_ppc_create": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _u64, C.POINTER(_vp)]),
    "lr_ppc_accumulate": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "lr_ppc_result": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "lr_ppc_terms": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "lr_ppc_reset": (C.c_int, [_vp]),
    "lr_ppc_destroy": (None, [_vp]),
}

_lib = None
_nuts = None
_pg = None
_hs = None
_dense = None
_factor = None
_predict = None
_acf = None
_marg = None
_loo = None
_bridge = None
_rank = None
_ppc = None
_cov = None
_adapt = None
_adapt_tall = None


def _bind(L, table, slot=None):
    """`L` (a loaded library handle) with the entry points of `table` bound; resolved once per handle, which the module global named
    `slot` remembers (no slot: resolved at every call)."""
    if slot is None or globals()[slot] is not L:
        for name, (res, args) in table.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the binding drift apart
            fn.restype = res
            fn.argtypes = args
        if slot is not None:
            globals()[slot] = L
    return L


def bind_nuts(L):
    """`L` (a loaded library handle) with the NUTS entry points bound; resolved once per handle."""
    return _bind(L, NUTS_SYMBOLS, "_nuts")


def load_nuts():
    """The library with the NUTS entry points bound (the same liblogreg_hip.so as load())."""
    return bind_nuts(load())


def bind_predict(L):
    """`L` (a loaded library handle) with the prediction entry points bound; resolved once per handle."""
    return _bind(L, PREDICT_SYMBOLS, "_predict")


def load_predict():
    """The library with the prediction entry points bound (the same liblogreg_hip.so as load())."""
    return bind_predict(load())


def bind_acf(L):
    """`L` (a loaded library handle) with the autocorrelation entry points bound; resolved once per handle."""
    return _bind(L, ACF_SYMBOLS, "_acf")


def load_acf():
    """The library with the autocorrelation entry points bound (the same liblogreg_hip.so as load())."""
    return bind_acf(load())


def bind_marginals(L):
    """`L` (a loaded library handle) with the marginals entry points bound; resolved once per handle."""
    return _bind(L, MARG_SYMBOLS, "_marg")


def load_marginals():
    """The library with the marginals entry points bound (the same liblogreg_hip.so as load())."""
    return bind_marginals(load())


def bind_loo(L):
    """`L` (a loaded library handle) with the PSIS-LOO entry points bound; resolved once per handle."""
    return _bind(L, LOO_SYMBOLS, "_loo")


def load_loo():
    """The library with the PSIS-LOO entry points bound (the same liblogreg_hip.so as load())."""
    return bind_loo(load())


def bind_bridge(L):
    """`L` (a loaded library handle) with the bridge-sampling entry points bound; resolved once per handle."""
    return _bind(L, BRIDGE_SYMBOLS, "_bridge")


def load_bridge():
    """The library with the bridge-sampling entry points bound (the same liblogreg_hip.so as load())."""
    return bind_bridge(load())


def bind_rank(L):
    """`L` (a loaded library handle) with the rank-diagnostics entry points bound; resolved once per handle."""
    return _bind(L, RANK_SYMBOLS, "_rank")


def load_rank():
    """The library with the rank-diagnostics entry points bound (the same liblogreg_hip.so as load())."""
    return bind_rank(load())


def bind_ppc(L):
    """`L` (a loaded library handle) with the predictive-check entry points bound; resolved once per handle."""
    return _bind(L, PPC_SYMBOLS, "_ppc")


def load_ppc():
    """The library with the predictive-check entry points bound (the same liblogreg_hip.so as load())."""
    return bind_ppc(load())


def bind_covariance(L):
    """`L` (a loaded library handle) with the covariance entry points bound; resolved once per handle."""
    return _bind(L, COV_SYMBOLS, "_cov")


def load_covariance():
    """The library with the covariance entry points bound (the same liblogreg_hip.so as load())."""
    return bind_covariance(load())


def bind_adapt(L):
    """`L` (a loaded library handle) with the NUTS warm-up entry points bound; resolved once per handle."""
    return _bind(L, ADAPT_SYMBOLS, "_adapt")


def load_adapt():
    """The library with the NUTS warm-up entry points bound (the same liblogreg_hip.so as load())."""
    return bind_adapt(load())


def bind_adapt_tall(L):
    """`L` (a loaded library handle) with the entry points of the NUTS warm-up on the stepwise engine bound, and those of the warm-up
    itself, which serve its handle; resolved once per handle."""
    return _bind(bind_adapt(L), ADAPT_TALL_SYMBOLS, "_adapt_tall")


def load_adapt_tall():
    """The library with the stepwise warm-up's entry points bound (the same liblogreg_hip.so as load())."""
    return bind_adapt_tall(load())


def bind_dense(L):
    """`L` (a loaded library handle) with the dense-metric NUTS entry points bound; resolved once per handle."""
    return _bind(L, DENSE_SYMBOLS, "_dense")


def load_dense():
    """The library with the dense-metric NUTS entry points bound (the same liblogreg_hip.so as load())."""
    return bind_dense(load())


def bind_pg(L):
    """`L` (a loaded library handle) with the Polya-Gamma entry points bound; resolved once per handle."""
    return _bind(L, PG_SYMBOLS, "_pg")


def load_pg():
    """The library with the Polya-Gamma entry points bound (the same liblogreg_hip.so as load())."""
    return bind_pg(load())


def bind_hs(L):
    """`L` (a loaded library handle) with the horseshoe Polya-Gamma entry points bound; resolved once per handle."""
    return _bind(L, HS_SYMBOLS, "_hs")


def load_hs():
    """The library with the horseshoe Polya-Gamma entry points bound (the same liblogreg_hip.so as load())."""
    return bind_hs(load())


def load():
    """Load the HIP library (building it first if the sources are newer and hipcc is present)."""
    global _lib
    if _lib is None:
        _lib = _open()
    return _lib


def load_factor():
    """liblogreg_hip.so itself with `lr_dense_factor` and `lr_last_error` bound.  The factorisation is host code with no device and no
    model behind it, so it does not follow a handle that was put in load()'s place: the CPU test doubles hold SYMBOLS alone, and a
    kernel object above one of their models still validates its matrix."""
    global _factor
    if _factor is None:
        L = _open()
        L.lr_dense_factor.restype, L.lr_dense_factor.argtypes = DENSE_SYMBOLS["lr_dense_factor"]
        _factor = L
    return _factor


def _open():
    """A checked handle of liblogreg_hip.so with SYMBOLS bound: current (rebuilt if stale), of these sources, of this binding's layout."""
    from . import build as _build
    if _build.built_extra() and _build.EXTRA_ENV not in os.environ:
        # a development build (e.g. -DLR_STAMPS: clock reads and printf in hot loops) left behind by a profiling tool must
        # never be what an ordinary run times or tests: replace it with the production build, or refuse
        try:
            _build.build(force=True, verbose=False)
        except Exception as e:
            raise LogregHipError(
                f"{LIB_PATH} is a development build (flags {_build.built_extra()!r}) and the production library could not be "
                f"rebuilt: {e}.  Run `python -m logreg_amd.build --force`, or set {_build.EXTRA_ENV} to use it on purpose.") from e
    if _build.needs_build():  # missing, or older than a kernel source / the header: never run stale kernels
        try:
            _build.build(verbose=False)
        except Exception as e:  # no hipcc / compile error: loud, no fallback
            raise LogregHipError(
                f"liblogreg_hip.so is missing or stale ({LIB_PATH}) and could not be built: {e}. "
                "Run `python -m logreg_amd.build`. There is no CPU fallback.") from e
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise LogregHipError(f"cannot load {LIB_PATH}: {e}. There is no CPU fallback.") from e
    _bind(L, SYMBOLS)  # (load() remembers the handle only once the checks below have passed)
    have, want = L.lr_build_id().decode(), _build.source_hash()
    if have != want:
        raise LogregHipError(f"{LIB_PATH} was built from other sources (build id {have}, sources {want}); "
                             "run `python -m logreg_amd.build --force`")
    if L.lr_sizeof_run_opts() != C.sizeof(RunOpts):
        raise LogregHipError(f"lr_run_opts is {L.lr_sizeof_run_opts()} bytes in the library, {C.sizeof(RunOpts)} in the binding")
    return L


def check(rc: int):
    if rc != 0:
        msg = load().lr_last_error()
        raise LogregHipError(f"liblogreg_hip error {rc}: {msg.decode() if msg else '?'}")


def device_count() -> int:
    return int(load().lr_device_count())


def device_info(device: int = 0) -> str:
    """"pci=... uuid=... name=... cus=..." of `device` (lr_device_info)."""
    buf = C.create_string_buffer(256)
    check(load().lr_device_info(int(device), buf, 256))
    return buf.value.decode()


def require_gpu():
    n = device_count()
    if n <= 0:
        raise LogregHipError("no AMD GPU visible to HIP: logreg_amd has no CPU fallback "
                             "(the CPU restatement under oracle/ is test infrastructure only)")
    return n
