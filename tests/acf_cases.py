"""The test set of the autocorrelation accumulator (include/logreg_hip_acf.h) -- TEST INFRASTRUCTURE ONLY.

Series: seeded AR(1), x_t = 3 + 0.5 z_t with z stationary of unit variance and phi in {0, 0.5, 0.9, 0.97} (series s of a case takes
PHIS[s % 4]), rounded to the dtype of the case.  From five chains on, a case also holds the special series: a constant one, one at an
offset of 1e4 sd (the pivot), one chain with a NaN and one with an inf.

Shapes (C, p, n, K): the smallest at which the kernel can go wrong -- C in {1, 5, 37, 130} and p in {1, 3, 8, 20} (no multiples of the
tile of 16 series; up to 163 workgroups), n in {1, 3, 5, 64, 200, 601} (and 7, 8, 63: n = K and n = K + 1 at K = 7, n = K at K = 63),
K in {1, 7, 63, 255} (n < K, n = K, n = K + 1; K > 63: a lane owns several lags; n = 200 and 601: more than one tile of 128 steps).
At phi = 0.97, n = 601 the truncation lag goes far beyond 63: capped series at K <= 63, uncapped ones at K = 255.

Feedings: one call, chunks of 1, 7, K, K + 1, uneven chunks; host and device memory.
"""
import numpy as np

PHIS = (0.0, 0.5, 0.9, 0.97)
DTYPES = ("float64", "float32")
SHAPES = [  # (C, p, n, K)
    (1, 1, 1, 1), (1, 3, 3, 7), (5, 1, 5, 1), (5, 3, 5, 7), (5, 3, 7, 7), (5, 3, 8, 7), (37, 3, 64, 7), (130, 1, 64, 1), (130, 8, 200, 7),
    (5, 3, 63, 63), (37, 8, 64, 63), (130, 20, 64, 63), (5, 20, 200, 63), (37, 1, 601, 63), (37, 20, 5, 63),
    (5, 8, 200, 255), (5, 3, 601, 255), (1, 8, 601, 255), (37, 3, 64, 255), (37, 8, 601, 255),
]
NAMES = [f"C{C}_p{p}_n{n}_K{K}" for C, p, n, K in SHAPES]
_CACHE = {}


def ar1(rng, phi, n):
    e = rng.standard_normal(n)
    z = np.empty(n)
    z[0] = e[0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        z[t] = phi * z[t - 1] + s * e[t]
    return 3.0 + 0.5 * z


def case(name, dtype):
    """-> dict(name, dtype, C, p, n, K, x [n, C, p] float64 holding values of `dtype`).  Cached; treat as read-only."""
    key = (name, dtype)
    if key not in _CACHE:
        idx = NAMES.index(name)
        C, p, n, K = SHAPES[idx]
        rng = np.random.default_rng(1000 + idx)
        x = np.empty((n, C, p))
        for c in range(C):
            for j in range(p):
                x[:, c, j] = ar1(rng, PHIS[(c * p + j) % 4], n)
        if C >= 5:
            x[:, 1, 0] = 3.0                      # constant
            x[:, 2, :] += 1e4 * 0.5               # offset of 1e4 sd: every coordinate of chain 2
            x[n // 2, 3, 0] = np.nan              # one NaN (chain 3, first coordinate)
            x[n - 1, 4, p - 1] = np.inf           # one inf, in the last draw (chain 4, last coordinate)
            if n > 1:
                x[0, 4, 0] = -np.inf              # ... and one in the first draw: the pivot itself (p = 1: the same series)
        x = x.astype(dtype).astype(np.float64)
        x.setflags(write=False)
        _CACHE[key] = dict(name=name, dtype=dtype, C=C, p=p, n=n, K=K, x=x)
    return _CACHE[key]


def chunkings(n, K):
    """-> [(label, [chunk lengths], memory)]"""
    def cut(k):
        return [k] * (n // k) + ([n % k] if n % k else [])
    uneven, left, i = [], n, 0
    pattern = (3, 1, 130, 2, 17, 64, 129, 5)
    while left > 0:
        k = min(pattern[i % len(pattern)], left)
        uneven.append(k)
        left -= k
        i += 1
    return [("one call", [n], "host"), ("one call", [n], "device"), ("chunks of 1", cut(1), "device"), ("chunks of 7", cut(7), "host"),
            (f"chunks of K={K}", cut(K), "device"), (f"chunks of K+1={K + 1}", cut(K + 1), "host"), ("uneven", uneven, "device"),
            ("uneven", uneven, "host")]


def feed(la, ac, x, lengths, memory):
    """Fold x [n, C, p] (already of the accumulator's dtype) into `ac` in chunks of `lengths`, from host or device memory."""
    assert sum(lengths) == x.shape[0]
    dev = la.DeviceArray.from_host(ac.device, x) if memory == "device" else None
    t = 0
    for k in lengths:
        ac.update(dev.rows(t, t + k) if dev is not None else x[t:t + k])
        t += k
    if dev is not None:
        ac.sums()  # (synchronises: the block may go)
        dev.free()
