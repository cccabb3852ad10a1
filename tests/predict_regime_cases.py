"""Cases of the draw-consuming kernels at saturated logits (tests/test_predict_regimes_cpu.py, tests/test_gpu_predict_regimes.py): the
posterior-predictive table (k_predict_partial) and the pointwise log-likelihood fill (k_loo_fill), which share pred_pair of
csrc/lr_predict.h.  Built on tests/eval_cases.py: its 8 shapes, its three designs and its ladder of max_i |t_i| = T.

Shapes (p, n) and what they reach in lr_predict.h (`draws_in_flight` restates PredGeom):  (3, 37) padded width 4; (8, 1) one real row, 255
lanes redo it; (8, 208); (12, 209) padded width 16, where float32 still holds 4 draws in flight and float64 holds 2; (17, 65) padded width
32: 2 draws in flight in float32, ONE in float64; (32, 257) the same on two tiles of 256 lanes; (40, 63) padded width 64: float64 takes the
chunked wide-row path (groups of 8), float32 holds the row in registers with one draw in flight; (128, 130) chunked in both dtypes.
The designs cycle so that plain, scaled and outlier each sit on an exact width (8, 8, 32), on a padded one (3, 12, 17) and on a chunked one (128, 40, 128): nine cases, (128, 130) twice.

Rows: most cases predict the model's own rows (X_new = None); p12_n209_scaled passes new rows with labels and p40_n63_outlier new rows
without (pi only; rows 2 - 4 of the table are NaN) -- the model's rows in reverse order with the last third dropped, so r != n.  The
log-likelihood fill always reads the model's own rows.

Draws, two sets per case:
  mixed    S = 134 draws walking eval_cases.PAIRS in order (four directions x T in 1, 30, 90, 130, 700, 5000), scaled by the
           prediction rows.  The host rules (lr_api.hip, restated in `predict_slices` / `fill_slices` and asserted by the CPU test): the
           accumulator cuts 134 draws into slices of 45, 45 and 44 -- a pivot, then 11 groups of 4 with nothing left, or 10 groups of 4
           and a remainder of 3 (groups of 8: 5 and a remainder of 4 or 3; groups of 2: 22, or 21 and 1) -- and the fill into slices of
           64, 64 and 6, the last one a partial tile.  Neighbouring draws, and so neighbouring slices, have means that differ by
           thousands: the pairwise merge's worst input.
  by rung  for each T in 30, 90, 130, 700, 5000: S = 9 draws -d* T j / max_i |x_i . d*|, j spread over [0.9, 1].  Every row is on the
           wrong side in every draw, so the mean of L is tiny wherever the row's margin is not, and only a relative check means anything.
           T = 90 puts float32 L inside the subnormal range (|t| in 87.3 ... 103.9), T = 5000 is past the float64 clamp at -750.
Each case runs under two of predict_cases.BATCHINGS that cut the draws alike -- one batch from host and from device memory on the even
cases, the uneven batches (1, 10, 73 and 50 of the 134 draws: later batches merge into a running table) on the odd ones -- so the two
tables must agree to the byte: the order of the merges is the same.
"""
import numpy as np

import eval_cases as ec

S_MIXED = 134
S_RUNG = 9
RUNGS = (30, 90, 130, 700, 5000)
DTYPES = ec.DTYPES
# (p, n, design, rows): rows = "own", "new" (X_new with y_new) or "nolabels"
LAYOUT = [(3, 37, "plain", "own"), (8, 1, "scaled", "own"), (8, 208, "outlier", "own"), (12, 209, "scaled", "new"), (17, 65, "outlier", "own"),
          (32, 257, "plain", "own"), (40, 63, "outlier", "nolabels"), (128, 130, "scaled", "own"), (128, 130, "plain", "own")]
NAMES = [f"p{p}_n{n}_{d}" for p, n, d, _ in LAYOUT]
SETS = ("mixed",) + tuple(f"T{T}" for T in RUNGS)
# Which draw of its design a case takes (default: the first), as eval_cases.DRAWS: tests/test_predict_regimes_cpu.py asks that plain
# sequential arithmetic in the model's dtype stay within 0.5 of every bound -- a condition on the inputs, never on the bounds.
DRAWS = {}
_CACHE = {}


def case(name):
    """dict(name, p, n, design, X, y, prior_sd (the model), X_new, y_new (None = the model's own), rows, labels (of the prediction rows, or
    None), sets {"mixed": B [134, p], "T30": B [9, p], ...}, pairs (direction, T) per draw of the mixed set, batchings)."""
    if name not in _CACHE:
        k = NAMES.index(name)
        p, n, kind, rows = LAYOUT[k]
        seed = 500 + k + 100 * DRAWS.get(name, 0)
        X, y, sd, dstar, scale, outlier = ec.design(p, n, kind, seed)
        if rows == "own":
            Xn, yn, X_new, y_new = X, y, None, None
        else:
            keep = n - n // 3
            Xn, yn = X[::-1][:keep].copy(), y[::-1][:keep].copy()
            X_new, y_new = Xn, (yn if rows == "new" else None)
            if y_new is None:
                yn = None
        sets = {"mixed": ec.betas(Xn, dstar, scale, seed, S_MIXED, ec.PAIRS)}
        j = np.linspace(0.9, 1.0, S_RUNG)
        for T in RUNGS:
            sets[f"T{T}"] = ec.betas(Xn, dstar, scale, seed, 1, [("minus", T)]) * j[:, None] + 0.0
        _CACHE[name] = dict(name=name, p=p, n=n, design=kind, X=X, y=y, prior_sd=sd, X_new=X_new, y_new=y_new, rows=Xn, labels=yn, kind=rows, sets=sets,
                            pairs=[ec.PAIRS[c % len(ec.PAIRS)] for c in range(S_MIXED)], dstar=dstar, outlier=outlier,
                            batchings=("host_uneven", "device_uneven") if k % 2 else ("host", "device"))
    return _CACHE[name]


def draws_in_flight(p, dtype):
    """PredGeom<T, P>::DG of csrc/lr_predict.h for the real width p: (padded width, draws per group, chunked?)."""
    P = next(w for w in (4, 8, 16, 32, 64, 128) if w >= p)
    dw = 1 if dtype == "float32" else 2
    if P * dw > 64:
        return P, 8, True
    return P, (4 if 4 * P * dw <= 64 else max(64 // (P * dw), 1)), False


def predict_slices(r, S, cus=256):
    """pred_slicing of csrc/lr_api.hip: the draw counts of the slices k_predict_partial walks."""
    tiles = (r + 255) // 256
    sl = max(1, min((cus * 4 + tiles - 1) // tiles, (S + 63) // 64))
    per = (S + sl - 1) // sl
    return [min(per, S - a) for a in range(0, S, per)]


def fill_slices(n, S, dtype, cus=256):
    """loo_fill of csrc/lr_api.hip: (the draw counts of the slices k_loo_fill walks, draws per tile)."""
    ts = 128 // (4 if dtype == "float32" else 8)
    tiles = (n + 255) // 256
    sl = max(1, (cus * 4 + tiles - 1) // tiles)
    per = max(64, (S + sl - 1) // sl)
    per = (per + ts - 1) // ts * ts
    return [min(per, S - a) for a in range(0, S, per)], ts


def reference(name, dtype, which, rows="pred"):
    """The per-pair reference of one set of draws of a case with its bounds (tests/pair_reference.py), cached: dict(ref, tol, table, ttol).
    rows = "pred": the prediction rows and their labels; rows = "model": the model's own rows and labels (what the fill reads)."""
    import pair_reference as pref
    c = case(name)
    if rows == "model" and c["kind"] == "own":
        rows = "pred"
    key = ("ref", name, dtype, which, rows)
    if key not in _CACHE:
        X, y = (c["rows"], c["labels"]) if rows == "pred" else (c["X"], c["y"])
        ref = pref.pairs(X, y, c["sets"][which], dtype)
        tol = pref.pair_bounds(ref)
        _CACHE[key] = dict(ref=ref, tol=tol, table=pref.table(ref), ttol=pref.table_bounds(ref, tol))
    return _CACHE[key]
