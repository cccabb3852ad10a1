"""The test set of the covariance accumulator (include/logreg_hip_cov.h) -- TEST INFRASTRUCTURE ONLY.

Draws: as tests/marginals_cases.py, seeded AR(1) (phi = 0.5) z of unit variance per series, then mixed by a fixed lower-triangular
matrix, y_0 = z_0, y_j = rho_j y_(j-1) + sqrt(1 - rho_j^2) z_j with rho_j cycling through 0.9, -0.9, 0.6, -0.4, 0, 0.8, -0.7 (unit
variances, neighbours correlated from -0.9 to 0.9), x = loc_j + scale_j y_j with the coordinates located from -3 to 40 and scaled from
0.01 to 10; rounded to the dtype of the case.  center and scale are the draws' own mean and 1 / sd, rounded to the dtype of the case.

Shapes (C, p, n), the smallest at which the kernel can go wrong (P = padded width, R = time residues, chunk = chains staged together):
    C37_p8_n64          P 8, groups of 16 chains: three, the last ragged (5 chains); n = 2 R + 14
    C5_p20_n200         p padded to 32 (12 zero columns), groups of 4: two, the last of one chain
    C1_p1_n7            one series; fewer time steps than residues
    C3_p128_n16         the widest tile (8 x 8 of 16 x 16 blocks, R = 1), fewer chains than a chunk
    C130_p3_n601        P 4, groups of 32: five; n = 24 R + 1, beyond any residue count and not a multiple of it
    C300_p1_n40         ten groups, one coordinate
    C37_p8_n64_same     EVERY draw is the same value: the covariance is 0 and cor is NaN
    C5000_p3_n3         157 groups of 32: 3925 cells, 62 runs of cells merged at result time
    C4100_p33_n9        P 64 (R = 7, chunk 8): more chains than 512 chunks, so groups of 16 = two chunks each; the last group ragged (4
                        chains); two windows of time steps
From five chains on a case holds the special series of the marginals set (jf = 1 where p >= 3, else 0):
    chain 1, jf      constant          chain 3, 0       one NaN          chain 4, p - 1      -inf in the first draw, +inf in the last
(not the `_same` case).

Feedings: those of marginals_cases.chunkings (one call, chunks of 1, of 7, uneven; host and device memory).
"""
import numpy as np

from marginals_cases import chunkings  # noqa: F401  (the feedings are the marginals')

DTYPES = ("float64", "float32")
SHAPES = {  # name -> (C, p, n)
    "C37_p8_n64": (37, 8, 64), "C5_p20_n200": (5, 20, 200), "C1_p1_n7": (1, 1, 7), "C3_p128_n16": (3, 128, 16),
    "C130_p3_n601": (130, 3, 601), "C300_p1_n40": (300, 1, 40), "C37_p8_n64_same": (37, 8, 64), "C5000_p3_n3": (5000, 3, 3),
    "C4100_p33_n9": (4100, 33, 9),
}
NAMES = list(SHAPES)
RHO = (0.9, -0.9, 0.6, -0.4, 0.0, 0.8, -0.7)
_CACHE = {}


def case(name, dtype):
    """-> dict(name, dtype, C, p, n, center, scale [p] float64, x [n, C, p] float64 holding values of `dtype`).  Cached; read-only."""
    key = (name, dtype)
    if key not in _CACHE:
        C, p, n = SHAPES[name]
        if name.endswith("_same"):
            x = np.full((n, C, p), 1.25)
            center, scale = np.ones(p), np.full(p, 2.0)
        else:
            rng = np.random.default_rng(3000 + NAMES.index(name))
            e = rng.standard_normal((n, C, p))
            z = np.empty((n, C, p))
            z[0] = e[0]
            for t in range(1, n):
                z[t] = 0.5 * z[t - 1] + np.sqrt(0.75) * e[t]
            y = np.empty_like(z)
            y[..., 0] = z[..., 0]
            for j in range(1, p):
                rho = RHO[(j - 1) % len(RHO)]
                y[..., j] = rho * y[..., j - 1] + np.sqrt(1.0 - rho * rho) * z[..., j]
            loc = np.linspace(-3.0, 40.0, p) if p > 1 else np.array([40.0])
            scl = np.geomspace(0.01, 10.0, p) if p > 1 else np.array([0.01])
            x = (loc + scl * y).astype(dtype).astype(np.float64)
            center = x.mean(axis=(0, 1)).astype(dtype).astype(np.float64)
            scale = (1.0 / x.std(axis=(0, 1))).astype(dtype).astype(np.float64)
            if C >= 5:
                jf = 1 if p >= 3 else 0
                x[:, 1, jf] = x[0, 1, jf]
                x[n // 2, 3, 0] = np.nan
                x[0, 4, p - 1] = -np.inf
                x[n - 1, 4, p - 1] = np.inf
        x.setflags(write=False)
        _CACHE[key] = dict(name=name, dtype=dtype, C=C, p=p, n=n, center=center, scale=scale, x=x)
    return _CACHE[key]


def feed(la, acc, x, lengths, memory):
    """Fold x [n, C, p] (already of the accumulator's dtype) into `acc` in chunks of `lengths`, from host or device memory."""
    assert sum(lengths) == x.shape[0]
    dev = la.DeviceArray.from_host(acc.device, x) if memory == "device" else None
    t = 0
    for k in lengths:
        acc.update(dev.rows(t, t + k) if dev is not None else x[t:t + k])
        t += k
    if dev is not None:
        acc.tables()  # (synchronises: the block may go)
        dev.free()
