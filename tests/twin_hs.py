"""Build and inject the CPU test double of the horseshoe Polya-Gamma ABI (tests/host/lr_cpu_twin_hs.c: the whole double of
tests/host/lr_cpu_twin_pg.c plus lr_run_hs and lr_hs_hyper) -- TEST INFRASTRUCTURE ONLY, modelled on tests/twin_pg.py.

`install()` compiles it into a temporary directory, binds the three symbol tables of the product's ctypes binding it serves
(logreg_amd/_lib.py SYMBOLS, PG_SYMBOLS and HS_SYMBOLS) and puts it where `logreg_amd._lib.load()` / `load_pg()` / `load_hs()` keep their
handle; `uninstall()` restores them.
"""
import ctypes as C
import os
import subprocess
import tempfile

import twin

REPO = twin.REPO
SRC = os.path.join(REPO, "tests", "host", "lr_cpu_twin_hs.c")
_state = {"dir": None, "path": None, "saved": None}


def build() -> str:
    """-> path of the double's shared library (built once per process)"""
    if _state["path"] is None:
        _state["dir"] = tempfile.TemporaryDirectory(prefix="lr_twin_hs_")
        path = os.path.join(_state["dir"].name, "liblogreg_twin_hs.so")
        r = subprocess.run(["gcc", *twin.CFLAGS, "-shared", SRC, "-o", path, "-lm", "-lrt", "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("building the horseshoe test double failed:\n" + r.stderr)
        _state["path"] = path
    return _state["path"]


def install():
    """Make `logreg_amd._lib.load()`, `load_pg()` and `load_hs()` return the double.  Returns the bound CDLL."""
    from logreg_amd import _lib
    L = C.CDLL(build())
    for table in (_lib.SYMBOLS, _lib.PG_SYMBOLS, _lib.HS_SYMBOLS):
        for name, (res, args) in table.items():
            fn = getattr(L, name)  # AttributeError if the double and the binding drift apart
            fn.restype = res
            fn.argtypes = args
    assert L.lr_sizeof_run_opts() == C.sizeof(_lib.RunOpts)
    if _state["saved"] is None:
        _state["saved"] = (_lib._lib, _lib._pg, _lib._hs)
    _lib._lib = L
    _lib._pg = L
    _lib._hs = L
    return L


def uninstall():
    import gc
    from logreg_amd import _lib
    gc.collect()
    if _state["saved"] is not None:
        _lib._lib, _lib._pg, _lib._hs = _state["saved"]
        _state["saved"] = None
