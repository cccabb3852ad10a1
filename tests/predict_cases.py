"""The test set of the posterior-predictive accumulator -- TEST INFRASTRUCTURE ONLY: one list of cases for tests/test_gpu_predict.py
and for its `--measure` mode, which prints the figures the test's bounds are derived from (profiles/r9_predict.txt).

Every real width maps to one padded width of the library: p = 3 -> 4, 8 -> 8, 13 -> 16, 20 -> 32, 32 -> 32, 47 -> 64, 128 -> 128.
Prediction-row counts r in {1, 63, 200, 1000, 4097} and draw counts S in {1, 255, 4096, 262144} all occur; the draws are posterior-like
(Laplace approximation around the posterior mode: predict_reference.posterior_like_draws)."""
import json
import os

import numpy as np

import predict_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHINGS = ("host", "host_uneven", "device", "device_uneven")


NAMES = ["pima_own_r200_S4096", "pima_new_r63_S262144", "pima_new_r1_S255_nolabels", "pima_own_r200_S1", "synthetic_p3_r1000_S4096",
         "synthetic_p8_r4097_S4096", "synthetic_p13_r4097_S255", "synthetic_p20_r63_S4096_nolabels", "synthetic_p32_r200_S4096",
         "synthetic_p47_r1000_S255", "synthetic_p128_r200_S4096", "synthetic_p128_r1_S255", "synthetic_own_p8_r1000_S4096"]  # of cases(), in order


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _synthetic(n, p, seed):
    from logreg_amd import synthetic_logreg
    return synthetic_logreg(n, p, seed=seed)[:2]


def cases():
    """-> list of dicts: name, X, y, pscale (the model), X_new / y_new (None = the model's own design), B [S, p] float64 draws,
    batchings (two of BATCHINGS: every case runs under both and both meet the reference)."""
    out = []
    d = _golden("pima_xy.json")
    Xp, yp = np.array(d["X"]), np.array(d["y"])
    ps = np.array(_golden("map.json")["pscale"])
    bmap = np.array(_golden("map.json")["map"])

    def pima_draws(S, seed):
        return pr.posterior_like_draws(Xp, yp, ps, S, seed, center=bmap)
    out.append(dict(name="pima_own_r200_S4096", X=Xp, y=yp, pscale=ps, X_new=None, y_new=None, B=pima_draws(4096, 1), batchings=("host", "device_uneven")))
    out.append(dict(name="pima_new_r63_S262144", X=Xp, y=yp, pscale=ps, X_new=Xp[:63], y_new=yp[:63], B=pima_draws(262144, 2),
                    batchings=("device", "host_uneven")))
    out.append(dict(name="pima_new_r1_S255_nolabels", X=Xp, y=yp, pscale=ps, X_new=Xp[100:101], y_new=None, B=pima_draws(255, 3),
                    batchings=("device", "host_uneven")))
    out.append(dict(name="pima_own_r200_S1", X=Xp, y=yp, pscale=ps, X_new=None, y_new=None, B=pima_draws(1, 4), batchings=("host", "device")))
    # (p, training rows, r, S, labels on the new rows)
    for p, n, r, S, lab in ((3, 300, 1000, 4096, True), (8, 500, 4097, 4096, True), (13, 400, 4097, 255, True), (20, 600, 63, 4096, False),
                            (32, 800, 200, 4096, True), (47, 2000, 1000, 255, True), (128, 4000, 200, 4096, True), (128, 4000, 1, 255, True)):
        X, y = _synthetic(n, p, 1000 + p)
        Xn, yn = _synthetic(r, p, 2000 + p + r)
        B = pr.posterior_like_draws(X, y, 1.0, S, 3000 + p)
        k = len(out)
        out.append(dict(name=f"synthetic_p{p}_r{r}_S{S}" + ("" if lab else "_nolabels"), X=X, y=y, pscale=np.ones(p), X_new=Xn, y_new=yn if lab else None, B=B,
                        batchings=(BATCHINGS[k % 4], BATCHINGS[(k + 2) % 4] if k % 2 else BATCHINGS[(k + 3) % 4])))
    X, y = _synthetic(1000, 8, 77)  # the model's own design once more, on the synthetic family and with a row count off the tile size
    out.append(dict(name="synthetic_own_p8_r1000_S4096", X=X, y=y, pscale=np.ones(8), X_new=None, y_new=None, B=pr.posterior_like_draws(X, y, 1.0, 4096, 78),
                    batchings=("device", "host_uneven")))
    assert [c["name"] for c in out] == NAMES
    return out


def rounded(case, np_dtype):
    """(rows, labels, draws) of a case as the model of dtype np_dtype sees them, back in float64: the reference's inputs."""
    Xn = case["X"] if case["X_new"] is None else case["X_new"]
    yn = case["y"] if case["X_new"] is None else case["y_new"]
    return Xn.astype(np_dtype).astype(np.float64), yn, case["B"].astype(np_dtype).astype(np.float64)


def uneven_splits(S):
    """Batch boundaries of an uneven batching of S draws (sizes 1, then growing, whatever is left at the end)."""
    edges, step = [0], 1
    while edges[-1] + step < S:
        edges.append(edges[-1] + step)
        step = step * 7 + 3
    edges.append(S)
    return list(zip(edges, edges[1:]))


def feed(la, pp, B, how):
    """Fold the draws B (already in the model's dtype) into pp under one of BATCHINGS."""
    model = pp.model
    pieces = [(0, B.shape[0])] if how in ("host", "device") else uneven_splits(B.shape[0])
    for a, b in pieces:
        blk = np.ascontiguousarray(B[a:b])
        if how.startswith("device"):
            d = la.DeviceArray.from_host(model.device, blk)
            pp.update(d)
            pp.table()  # (synchronises before the block is freed)
            d.free()
        else:
            pp.update(blk)
    return pp


def deviations(table, ref, S):
    """(mean rows, variance rows): the largest |difference| over rows 0, 2, 3, and over rows 1, 4 divided by S (a variance's scale).
    Entries that are NaN in both (no labels) count as equal; a NaN on one side only is infinite."""
    both = np.isnan(table) & np.isnan(ref)
    d = np.where(both, 0.0, np.abs(table - ref))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d[[0, 2, 3]].max()), float(d[[1, 4]].max() / S)
