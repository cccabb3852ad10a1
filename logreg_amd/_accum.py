"""What the accumulators of kept draws share on the Python face (the host scaffold under them is csrc/lr_accum.h).

`BlockAccumulator`   `Autocorr`, `Marginals`, `Covariance`, `RankDiagnostics` (which stores its blocks, and so also checks for room): blocks `[k, C, p]` in time order, created on a device at the first `update`, freed by `free`
`ModelAccumulator`   `PosteriorPredictive`, `PsisLoo`, `Bridge`, `PredictiveCheck`: draws `[S, p]` of a `LogReg`, created with the model, closed by `close`

A subclass names its entry points (`_prefix`: `<prefix>_accumulate`, `_reset`, `_destroy` of the C ABI) and supplies what really differs:
its constructor's own checks, the create call and the results.  `mcmc` asks every accumulator it is given `check_run` before anything runs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .model import _DTYPES, DeviceArray


class BlockAccumulator:
    """`chains` x `p` series of `dtype` draws on `device`, fed `[k, C, p]` blocks.  A subclass sets `_prefix`, `_bind` (the name of its
    bind function in _lib), `_entry_points` (for the error of a library without them) and `_keyword` (its name in `mcmc`), and defines
    `_create(L, out)` -> the return code of its create call."""

    def __init__(self, chains, p, dtype, device, **sizes):
        self._h = None
        self._L = None
        self._freed = False
        key = dtype
        if not (isinstance(dtype, str) and dtype in _DTYPES):
            try:
                key = np.dtype(dtype).name
            except TypeError:
                key = None
        if key not in _DTYPES:
            raise ValueError(f"dtype must be float32 or float64; got {dtype!r}")
        self.lr_dtype, self.np_dtype = _DTYPES[key]
        self.chains, self.p = int(chains), int(p)
        for name, value in sizes.items():  # (max_lag, bins: the subclass checks their range)
            setattr(self, name, int(value))
        self.device = int(device)
        if self.chains <= 0 or self.p <= 0:
            raise ValueError(f"chains and p must be positive; got {chains}, {p}")
        self.n_draws = 0

    @property
    def dtype(self):
        return np.dtype(self.np_dtype)

    @property
    def handle(self):
        if self._freed:
            raise _lib.LogregHipError("accumulator was freed")
        if self._h is None:
            L = _lib.load()
            _lib.require_gpu()  # no CPU path
            try:
                L = getattr(_lib, self._bind)(L)
            except AttributeError as e:
                raise _lib.LogregHipError(f"this library has no {self._entry_points}: {e}") from e
            h = C.c_void_p()
            check(self._create(L, C.byref(h)))
            self._L, self._h = L, h
        return self._h

    def check_block(self, shape, dtype=None, device=None):
        """Raise ValueError unless a block of this shape (and, for a DeviceArray, dtype and device) can be folded in."""
        shape = tuple(shape)
        if len(shape) != 3 or shape[1:] != (self.chains, self.p):
            raise ValueError(f"block must be [k, C, p] with C={self.chains}, p={self.p}; got {shape}")
        if shape[0] == 0:
            raise ValueError("block holds no draw (k = 0)")
        if dtype is not None and (np.dtype(dtype) != self.dtype or device != self.device):
            raise ValueError(f"a DeviceArray block must have dtype {self.dtype.name} on device {self.device}; got {np.dtype(dtype).name} on device {device}")

    def check_run(self, chains, model, iters):
        """Raise ValueError unless the kept draws of a run of `chains` chains of `model` can be folded in (`mcmc`, before anything runs)."""
        want = (int(chains), model.p, np.dtype(model.np_dtype), model.device)
        if (self.chains, self.p, self.dtype, self.device) != want:
            raise ValueError(f"{self._keyword}= is for {self.chains} chains x p={self.p} of {self.dtype.name} on device {self.device}; "
                             f"this run has {want[0]} chains x p={want[1]} of {want[2].name} on device {want[3]}")

    def update(self, block, stream=None):
        """Fold the next `k` time steps in: `[k, C, p]`, an ndarray (any float type; converted to the accumulator's dtype) or a
        `DeviceArray` of its dtype (enqueued on `stream`; the array may be freed once the stream has passed).  Returns self."""
        if isinstance(block, DeviceArray):
            self.check_block(block.shape, block.dtype, block.device)
            ptr, on_device = block.ptr, 1
        else:
            block = np.asarray(block)
            self.check_block(block.shape)
            if block.dtype.kind not in "fiu":
                raise ValueError(f"block must hold real numbers; got dtype {block.dtype}")
            a = np.ascontiguousarray(block, dtype=self.np_dtype)
            ptr, on_device = a.ctypes.data, 0
        h = self.handle
        check(getattr(self._L, self._prefix + "_accumulate")(h, ptr, int(block.shape[0]), on_device, stream))
        self.n_draws += int(block.shape[0])
        return self

    def reset(self):
        if self._h is not None:
            check(getattr(self._L, self._prefix + "_reset")(self._h))
        self.n_draws = 0

    def free(self):
        if getattr(self, "_h", None) is not None:
            getattr(self._L, self._prefix + "_destroy")(self._h)
            self._h = None
        self._freed = True

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ModelAccumulator:
    """Draws of `self.model` (a `LogReg`), fed `[S, p]` or `[iters, C, p]`; `self._L` is the library handle that made the model and
    `self._h` the accumulator the subclass created on it.  A subclass sets `_prefix` and defines `_library_count()` -> the draws the
    library holds (None if it cannot say); it may define `_check_room(S)` to refuse `S` more draws."""

    @property
    def handle(self):
        if self._h is None:
            raise _lib.LogregHipError("accumulator was closed")
        return self._h

    def _check_room(self, S):
        pass

    def update(self, draws, stream=None):
        """Fold draws in: `[S, p]` or `[iters, C, p]`, an ndarray (any float type; converted to the model's dtype) or a `DeviceArray`
        of the model's dtype (enqueued on `stream`; the array may be freed once the stream has passed).  More than the accumulator
        can hold (`PsisLoo`: `max_draws` in all) is refused and leaves it as it was.  Returns self."""
        m = self.model
        m.handle  # (raises if the model was closed: the accumulator reads the model's rows)
        shape = draws.shape if isinstance(draws, DeviceArray) else np.shape(draws)
        if len(shape) not in (2, 3) or shape[-1] != m.p:
            raise ValueError(f"draws must be [S, p] or [iters, C, p] with p={m.p}; got {tuple(shape)}")
        S = int(np.prod(shape[:-1], dtype=np.int64))
        if S == 0:
            raise ValueError("draws holds no draw (S = 0)")
        self._check_room(S)
        if isinstance(draws, DeviceArray):
            if draws.dtype != np.dtype(m.np_dtype) or draws.device != m.device:
                raise ValueError(f"a DeviceArray of draws must have the model's dtype {np.dtype(m.np_dtype).name} and device {m.device}; "
                                 f"got {draws.dtype.name} on device {draws.device}")
            ptr, on_device = draws.ptr, 1
        else:
            a = np.ascontiguousarray(draws, dtype=m.np_dtype)
            ptr, on_device = a.ctypes.data, 0
        rc = getattr(self._L, self._prefix + "_accumulate")(self.handle, ptr, S, on_device, stream)
        if rc == 0:
            self.n_draws += S
        else:  # a device error part-way: the library's count (the pieces it did take) is the one that holds
            try:
                check(rc)
            finally:
                n = self._library_count()
                if n is not None:
                    self.n_draws = n
        return self

    def close(self):
        if getattr(self, "_h", None) is not None:
            getattr(self._L, self._prefix + "_destroy")(self._h)  # (safe after the model was closed: the accumulator frees its own buffers only)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
