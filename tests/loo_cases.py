"""The test sets of PSIS-LOO -- TEST INFRASTRUCTURE ONLY: one list of cases each for the fill stage, the PSIS stage and the closed-form
guard, shared by tests/test_loo_cpu.py, tests/test_gpu_loo.py and the latter's `--measure` mode (profiles/r14_loo.txt).

Fill: every real width maps to one padded width of the library (p = 3 -> 4, 8 -> 8, 13 -> 16, 20 -> 32, 47 -> 64, 128 -> 128); n in
{1, 63, 257} (one lane, less than a wave's worth of a tile, more than one workgroup), S in {1, 24, 255, 1000} (1000 = more than one
slice with a partial last tile); every case under two of the four batchings of tests/predict_cases.py.
PSIS: Pima at S = 25, 255, 4096 and two synthetic models at S = 4096; the draws are posterior-like (Laplace approximation:
predict_reference.posterior_like_draws)."""
import numpy as np

import predict_cases as pc
import predict_reference as pr

# (p, n, S)
FILL = [(3, 257, 1000), (8, 63, 255), (13, 1, 24), (20, 257, 1), (47, 63, 1000), (128, 257, 255), (8, 1, 1000), (13, 257, 24)]
FILL_NAMES = [f"p{p}_n{n}_S{S}" for p, n, S in FILL]
PSIS_NAMES = ["pima_S25", "pima_S255", "pima_S4096", "synthetic_n60_p32_S4096", "synthetic_n300_p3_S4096"]
CLOSED_FORM_NAMES = ["pima_S25", "pima_S64", "pima_S255", "pima_S4096", "synthetic_n30_p20_S1000", "synthetic_n40_p13_S255",
                     "synthetic_n300_p3_S4096", "synthetic_n60_p32_S4096"]
DETERMINISM_NAMES = ["p3_n257_S1000", "p13_n257_S24", "p128_n257_S255"]  # a narrow, a padded and a wide p
TAIL_LENGTHS = {1: 0, 4: 0, 5: 1, 24: 4, 25: 5, 26: 5, 255: 48, 4096: 192, 1 << 20: 3072}  # S -> M; the cutoff is ascending index S - M - 1
_cache = {}


def _synthetic(n, p, seed):
    from logreg_amd import synthetic_logreg
    return synthetic_logreg(n, p, seed=seed)[:2]


def fill_case(name):
    """-> dict: name, X, y, pscale, B [S, p] float64 draws, batchings (two of predict_cases.BATCHINGS)"""
    if name not in _cache:
        k = FILL_NAMES.index(name)
        p, n, S = FILL[k]
        X, y = _synthetic(n, p, 500 + 7 * k)
        B = pr.posterior_like_draws(X, y, 1.0, S, 900 + k)
        _cache[name] = dict(name=name, X=X, y=y, pscale=np.ones(p), B=B, batchings=(pc.BATCHINGS[k % 4], pc.BATCHINGS[(k + 2) % 4] if k % 2 else pc.BATCHINGS[(k + 3) % 4]))
    return _cache[name]


def model_case(name):
    """A case of PSIS_NAMES / CLOSED_FORM_NAMES -> dict: name, X, y, pscale, B"""
    if name not in _cache:
        if name.startswith("pima_S"):
            d = pc._golden("pima_xy.json")
            X, y = np.array(d["X"]), np.array(d["y"])
            ps, bmap = np.array(pc._golden("map.json")["pscale"]), np.array(pc._golden("map.json")["map"])
            S = int(name[len("pima_S"):])
            B = pr.posterior_like_draws(X, y, ps, S, 40 + S, center=bmap)
        else:
            n, p, S = (int(t[1:]) for t in name.split("_")[1:])
            X, y = _synthetic(n, p, 100 + p)
            ps = np.ones(p)
            B = pr.posterior_like_draws(X, y, 1.0, S, 200 + p)
        _cache[name] = dict(name=name, X=X, y=y, pscale=ps, B=B)
    return _cache[name]


def rounded(case, np_dtype):
    """(rows, labels, draws) as the model of dtype np_dtype sees them, back in float64"""
    return case["X"].astype(np_dtype).astype(np.float64), case["y"], case["B"].astype(np_dtype).astype(np.float64)

