"""The shapes and inputs of the rank-diagnostics tests (tests/test_rank_cpu.py on the CPU double, tests/test_gpu_rank.py on the device).

Shapes (n, C, p), S = 2 (n // 2) C used draws per coordinate:
    (9, 3, 1)       S = 24: inside one wave, an odd n
    (64, 5, 3)      S = 320
    (130, 67, 2)    S = 8710: just past one LDS tile of 8192 keys, not a power of two
    (258, 509, 2)   S = 131 322: a sort padded to 2^18, five merges with global strides
Inputs: every entry is representable in the dtype asked for, so the float64 reference sees what the device stores.
"""
import numpy as np

SHAPES = [(9, 3, 1), (64, 5, 3), (130, 67, 2), (258, 509, 2)]
DTYPES = ["float32", "float64"]
RANK_KINDS = ["smooth", "sticky", "equal", "zeros", "denormal", "lastbit"]
STAT_KINDS = ["smooth", "sticky", "ar"]


def _seed(shape, kind, dtype):
    return [shape[0], shape[1], shape[2], RANK_KINDS.index(kind) if kind in RANK_KINDS else 17, DTYPES.index(dtype)]


def draws(shape, kind, dtype):
    """-> x [n, C, p] float64 holding values of `dtype`"""
    n, C, p = shape
    rng = np.random.default_rng(_seed(shape, kind, dtype))
    dt = np.dtype(dtype)
    if kind == "smooth":  # chains around slightly different places, a posterior far from 0
        x = 3.0 + rng.standard_normal((n, C, p)) + 0.05 * rng.standard_normal((1, C, p))
    elif kind == "sticky":  # every value repeated 10 times, as a random-walk sampler that rejects gives
        base = rng.standard_normal(((n + 9) // 10, C, p))
        x = np.repeat(base, 10, axis=0)[:n]
    elif kind == "ar":  # autocorrelated chains: a pair scan that runs a few pairs
        x = np.empty((n, C, p))
        x[0] = rng.standard_normal((C, p))
        for t in range(1, n):
            x[t] = 0.7 * x[t - 1] + rng.standard_normal((C, p))
    elif kind == "equal":  # coordinate 0 all equal; the others smooth
        x = rng.standard_normal((n, C, p))
        x[:, :, 0] = 1.5
    elif kind == "zeros":  # -0.0 and +0.0 mixed among a few other values: they tie
        x = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0, 0.25]), size=(n, C, p))
    elif kind == "denormal":  # multiples of the dtype's smallest denormal, both signs
        tiny = float(np.nextafter(dt.type(0), dt.type(1)))
        x = rng.integers(-40, 41, size=(n, C, p)).astype(np.float64) * tiny
    elif kind == "lastbit":  # neighbours in the dtype: values that differ in the last bit only
        eps = float(np.finfo(dt).eps)
        x = 1.0 + rng.integers(0, 6, size=(n, C, p)).astype(np.float64) * eps
    else:
        raise ValueError(kind)
    x = x.astype(dt).astype(np.float64)
    return x


def feedings(n):
    """[(label, chunk lengths, memory)]: one call, single steps, uneven chunks; host and device memory"""
    uneven = []
    left, k = n, 1
    while left:
        uneven.append(min(k, left))
        left -= uneven[-1]
        k = k * 2 + 1
    return [("one", [n], "host"), ("one", [n], "device"), ("steps", [1] * n, "host"), ("uneven", uneven, "device"), ("uneven", uneven, "host")]


def feed(la, acc, x, lengths, memory):
    """x [n, C, p] in the accumulator's dtype, in chunks of `lengths`, from host arrays or DeviceArrays"""
    assert sum(lengths) == x.shape[0]
    dev = la.DeviceArray.from_host(acc.device, np.ascontiguousarray(x)) if memory == "device" else None
    t = 0
    for k in lengths:
        acc.update(dev.rows(t, t + k) if dev is not None else x[t:t + k])
        t += k
    if dev is not None:
        acc.table()  # (synchronises: the block may go)
        dev.free()
