"""The test set of the marginals accumulator (include/logreg_hip_marginals.h) -- TEST INFRASTRUCTURE ONLY.

Draws: seeded AR(1) (phi = 0.5) z of unit variance, made skew, x = loc_j + scale_j (exp(0.4 z) - 1) / 0.4, with the coordinates located
from -3 to 40 and scaled from 0.01 to 10; rounded to the dtype of the case.  The grid of coordinate j is mean_j - 2.5 sd_j .. mean_j + 6 sd_j
of those draws (so the overflow column is populated), its ends rounded to the dtype of the case (a draw can equal them).

Shapes (C, p, n, B), the smallest at which the kernel can go wrong:
    C37_p8_n64_B64       two workgroups with a ragged tail
    C5_p20_n200_B256     p does not divide the workgroup width
    C130_p3_n601_B1024   the largest table that fits the LDS budget
    C1_p1_n7_B8          one series
    C3_p128_n16_B1024    a table beyond the LDS budget: the tiled lane map
    C300_p1_n40_B1       one bin, one coordinate, every lane of a workgroup on the same three counters
    C37_p8_n64_B64_same  EVERY draw of the block is the same value: all lanes on one counter
From five chains on a case holds the special series, in fixed places (jf = 1 where p >= 3, else 0: a coordinate that stays finite):
    chain 1, jf      constant
    chain 2, jf      draws exactly lo, exactly hi, the largest representable value below hi, one underflow and one overflow draw
    chain 3, 0       one NaN                          chain 4, p - 1      -inf in the first draw, +inf in the last

Feedings: one call, chunks of 1, chunks of 7, uneven chunks; host and device memory.
"""
import numpy as np

DTYPES = ("float64", "float32")
SHAPES = {  # name -> (C, p, n, B)
    "C37_p8_n64_B64": (37, 8, 64, 64), "C5_p20_n200_B256": (5, 20, 200, 256), "C130_p3_n601_B1024": (130, 3, 601, 1024),
    "C1_p1_n7_B8": (1, 1, 7, 8), "C3_p128_n16_B1024": (3, 128, 16, 1024), "C300_p1_n40_B1": (300, 1, 40, 1),
    "C37_p8_n64_B64_same": (37, 8, 64, 64),
}
NAMES = list(SHAPES)
QS = (0.0, 0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 1.0)
_CACHE = {}


def case(name, dtype):
    """-> dict(name, dtype, C, p, n, B, lo, hi [p] float64, x [n, C, p] float64 holding values of `dtype`).  Cached; read-only."""
    key = (name, dtype)
    if key not in _CACHE:
        C, p, n, B = SHAPES[name]
        if name.endswith("_same"):
            x = np.full((n, C, p), 1.25)
            lo, hi = np.zeros(p), np.full(p, 2.0)
        else:
            rng = np.random.default_rng(2000 + NAMES.index(name))
            e = rng.standard_normal((n, C, p))
            z = np.empty((n, C, p))
            z[0] = e[0]
            for t in range(1, n):
                z[t] = 0.5 * z[t - 1] + np.sqrt(0.75) * e[t]
            loc = np.linspace(-3.0, 40.0, p) if p > 1 else np.array([40.0])
            scale = np.geomspace(0.01, 10.0, p) if p > 1 else np.array([0.01])
            x = loc + scale * (np.exp(0.4 * z) - 1.0) / 0.4
            x = x.astype(dtype).astype(np.float64)
            mean, sd = x.mean(axis=(0, 1)), x.std(axis=(0, 1))
            lo = (mean - 2.5 * sd).astype(dtype).astype(np.float64)
            hi = (mean + 6.0 * sd).astype(dtype).astype(np.float64)
            if C >= 5:
                jf = 1 if p >= 3 else 0
                x[:, 1, jf] = x[0, 1, jf]                                   # constant
                below = np.nextafter(np.asarray(hi[jf], dtype=dtype), np.asarray(-np.inf, dtype=dtype))
                x[0:5, 2, jf] = [lo[jf], hi[jf], float(below), lo[jf] - 3.0 * sd[jf], hi[jf] + 2.0 * sd[jf]]
                x[n // 2, 3, 0] = np.nan
                x[0, 4, p - 1] = -np.inf
                x[n - 1, 4, p - 1] = np.inf
                x = x.astype(dtype).astype(np.float64)
        x.setflags(write=False)
        _CACHE[key] = dict(name=name, dtype=dtype, C=C, p=p, n=n, B=B, lo=lo, hi=hi, x=x)
    return _CACHE[key]


def chunkings(n):
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
            ("uneven", uneven, "device"), ("uneven", uneven, "host")]


def feed(la, mg, x, lengths, memory):
    """Fold x [n, C, p] (already of the accumulator's dtype) into `mg` in chunks of `lengths`, from host or device memory."""
    assert sum(lengths) == x.shape[0]
    dev = la.DeviceArray.from_host(mg.device, x) if memory == "device" else None
    t = 0
    for k in lengths:
        mg.update(dev.rows(t, t + k) if dev is not None else x[t:t + k])
        t += k
    if dev is not None:
        mg.counts_table()  # (synchronises: the block may go)
        dev.free()
