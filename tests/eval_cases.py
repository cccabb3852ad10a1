"""Cases of the model evaluation at saturated logits (tests/test_eval_regimes_cpu.py, tests/test_gpu_eval_regimes.py): the
smallest shapes at which each row layout can go wrong, three designs, and 65 parameter vectors per case that walk a ladder of
max_i |t_i| = T from the posterior's own range to both sides of every clamp in the device code.

Shapes (p, n):  (3, 37) the scalar dot product; (8, 1) one real row, the rest padding; (8, 208) 13 rows per lane on 16 lanes (product
form of the value) and 4 rows per lane on 64 (per-row form); (12, 209) padded width 16 and the lone row of the pair layout; (17, 65) and
(32, 257) the float64 distributed-state kernel; (40, 63) and (128, 130) the wide kernels.
Designs (column 0 is the intercept):  plain N(0, 1) entries; scaled: columns times 10^U(-3, 3) with beta compensated, from p = 8 one column
all zero and two rows duplicated; outlier: plain with one row times 1000, so that a single lane overflows its product.
prior_sd is log-uniform in [1e-2, 1e2].  Labels y = [X d* > 0] for a fixed d*, so d* separates the data; the case "ones" (p = 3, n = 37: the per-lane product form on 16 lanes x 16 rows) has all y = 1.
Chains: chain c takes the (direction, T) pair c mod 24 and beta = direction * T / max_i |x_i . direction|.  Directions: +d* (every t_i > 0,
ll in (-n log 2, 0]), -d* (every t_i < 0), a random direction (a new one per chain), the intercept alone.  T: 1; 30; 90 (float32 exp
overflows); 130 (2^ts past 2^127 and past the clamp at 100); 700 and 5000 (either side of the float64 clamp at -750).
"""
import itertools

import numpy as np

SHAPES = [(3, 37), (8, 1), (8, 208), (12, 209), (17, 65), (32, 257), (40, 63), (128, 130)]
DESIGNS = ("plain", "scaled", "outlier")
DIRECTIONS = ("plus", "minus", "random", "intercept")
T_LADDER = (1, 30, 90, 130, 700, 5000)
PAIRS = list(itertools.product(DIRECTIONS, T_LADDER))
CHAINS = 65
DTYPES = ("float32", "float64")
ONES = "p3_n37_ones"
NAMES = [f"p{p}_n{n}_{d}" for p, n in SHAPES for d in DESIGNS] + [ONES]
# Which draw of its design a case takes (default: the first).  tests/test_eval_regimes_cpu.py asks that plain sequential float32 arithmetic stay
# within 0.5 of every bound on every case -- a condition on the inputs, not on the bounds.  At n >= 208 the chains of the intercept direction
# put it near 0.5 whatever the draw (every |t_i| equal: n row terms of one or two values, whose sequential float32 sum errs systematically;
# largest ratio over the first 150 draws: 0.42 - 0.66), so these cases take a draw that keeps it low: at n = 208 and 209, of the first 150
# draws, the one with the smallest largest ratio (0.46, 0.46, 0.47; 0.43, 0.42, 0.43), at n = 257 the first under 0.42.  The all-ones case sits at n = 37 for the same reason: with one label every row term of an
# intercept chain is the same number, and at n = 208 no draw moves its ratio (0.58).
DRAWS = {"p8_n208_plain": 122, "p8_n208_scaled": 23, "p8_n208_outlier": 92, "p12_n209_plain": 32, "p12_n209_scaled": 61, "p12_n209_outlier": 136,
         "p32_n257_plain": 9, "p32_n257_scaled": 3, "p32_n257_outlier": 24}
_CACHE = {}


def design(p, n, kind, seed):
    """X [n, p], y [n], prior_sd [p], and the compensated separating direction d*, column scales and outlier row (or -1)."""
    rng = np.random.default_rng([20250022, seed, p, n])
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    dstar = rng.standard_normal(p)
    scale = np.ones(p)
    outlier = -1
    if kind == "scaled":
        scale[1:] = 10.0 ** rng.uniform(-3, 3, p - 1)
        X = X * scale
        if p >= 8:
            X[:, p // 2] = 0.0
            if n >= 4:
                X[n - 1], X[n - 2] = X[0], X[1]
    elif kind == "outlier":
        outlier = n // 2
        X[outlier, 1:] *= 1000.0
    dstar = dstar / scale
    y = (X @ dstar > 0).astype(np.float64)
    prior_sd = 10.0 ** rng.uniform(-2, 2, p)
    return X, y, prior_sd, dstar, scale, outlier


def betas(X, dstar, scale, seed, chains=CHAINS, pairs=PAIRS):
    rng = np.random.default_rng([20250023, seed, X.shape[1], X.shape[0]])
    p = X.shape[1]
    out = np.empty((chains, p))
    for c in range(chains):
        which, T = pairs[c % len(pairs)]
        d = {"plus": dstar, "minus": -dstar, "random": rng.standard_normal(p) / scale, "intercept": np.eye(p)[0]}[which]
        out[c] = d * (T / np.max(np.abs(X @ d))) + 0.0  # (+ 0.0: no negative zero, which x + 0 * z would not give back)
    return out


def case(name):
    """dict(name, p, n, design, X, y, prior_sd, beta [65, p], pairs [(direction, T)] per chain, dstar, outlier)."""
    if name not in _CACHE:
        ps, ns, kind = name.split("_")
        p, n = int(ps[1:]), int(ns[1:])
        ones = kind == "ones"
        seed = NAMES.index(name) + 100 * DRAWS.get(name, 0)
        X, y, sd, dstar, scale, outlier = design(p, n, "plain" if ones else kind, seed)
        if ones:
            y = np.ones(n)
        _CACHE[name] = dict(name=name, p=p, n=n, design=kind, X=X, y=y, prior_sd=sd, beta=betas(X, dstar, scale, seed),
                            pairs=[PAIRS[c % len(PAIRS)] for c in range(CHAINS)], dstar=dstar, outlier=outlier)
    return _CACHE[name]


# lr_hessian: p x n straddling the 64-row blocks of k_hess_partial; p = 128 is its largest LDS request
HESS_P = (3, 8, 33, 128)
HESS_N = (1, 63, 64, 65, 257)
HESS_DESIGNS = ("plain", "scaled")
HESS_T = (1, 30, 700)
HESS_NAMES = [f"p{p}_n{n}_{d}" for p in HESS_P for n in HESS_N for d in HESS_DESIGNS]


def hessian_case(name):
    """As case(), with three parameter vectors: the random direction at T = 1, +d* at T = 30, -d* at T = 700."""
    key = "hess_" + name
    if key not in _CACHE:
        ps, ns, kind = name.split("_")
        p, n = int(ps[1:]), int(ns[1:])
        seed = 1000 + HESS_NAMES.index(name)
        X, y, sd, dstar, scale, _ = design(p, n, kind, seed)
        pairs = [("random", 1), ("plus", 30), ("minus", 700)]
        _CACHE[key] = dict(name=name, p=p, n=n, design=kind, X=X, y=y, prior_sd=sd, beta=betas(X, dstar, scale, seed, 3, pairs), pairs=pairs)
    return _CACHE[key]
