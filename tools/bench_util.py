"""What the accumulator benchmarks (acf_bench.py, marginals_bench.py, predict_bench.py) share: event timing through the library's own
event calls, and the two repeat protocols."""
import ctypes as C

import numpy as np

from logreg_amd import _lib


class Events:
    def __init__(self, L, device, stream=None):
        self.L, self.device, self.stream = L, device, stream
        self.a, self.b = C.c_void_p(), C.c_void_p()
        _lib.check(L.lr_event_create(device, C.byref(self.a)))
        _lib.check(L.lr_event_create(device, C.byref(self.b)))

    def time(self, fn):
        ms = C.c_float()
        _lib.check(self.L.lr_event_record(self.device, self.a, self.stream))
        fn()
        _lib.check(self.L.lr_event_record(self.device, self.b, self.stream))
        _lib.check(self.L.lr_event_elapsed_ms(self.device, self.a, self.b, C.byref(ms)))
        return ms.value * 1e-3


def repeats(timer, fn, before=None, n=10):
    """n timed runs after a warm one, `before()` ahead of each"""
    out = []
    for i in range(n + 1):  # the first is the warm run
        if before is not None:
            before()
        t = timer(fn)
        if i:
            out.append(t)
    return np.array(out)


def repeats_until(timer, fn, min_total=0.5, min_n=5, max_n=200):
    """timed runs after a warm one until they add up to min_total seconds: at least min_n, at most max_n"""
    fn_time = []
    timer(fn)  # warm
    while (sum(fn_time) < min_total or len(fn_time) < min_n) and len(fn_time) < max_n:
        fn_time.append(timer(fn))
    return np.array(fn_time)
