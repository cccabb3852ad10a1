"""How the stand-alone host harnesses under tests/host/ are built and run -- stated once.  A harness is a program with its own main
that drives the C ABI on the stub HIP runtime (tests/host/hip_stub.cpp): it is linked with the stub, with lr_api.hip compiled for the
host under a named set of sanitizer flags, and with the library's own twelve instantiation objects.  The stub and lr_api.hip are
compiled once per flag set and process (one lr_api.hip compile is some thirty seconds), a harness once per (source, flag set); the
objects live in a temporary directory that goes when the process does, so nothing is ever stale.  Code loaded into Python is not
built here: the sanitized executables are these programs alone."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import REPO

CXX = "/opt/rocm/lib/llvm/bin/clang++"
HOST = os.path.join(REPO, "tests", "host")
FLAG_SETS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"], "plain": []}
INC = ["-I", os.path.join(REPO, "logreg_amd", "csrc"), "-I", os.path.join(REPO, "include")]
COMMON = ["-O1", "-g", "-std=c++17", *INC, "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-Wno-unused-function"]
RUN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0")
REPORTS = ("ERROR: AddressSanitizer", "LeakSanitizer", "runtime error", "WARNING: ThreadSanitizer")


@functools.lru_cache(maxsize=None)
def _tmp():
    d = tempfile.mkdtemp(prefix="lr_host_build_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _do(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _xarch_host(flags):
    return [a for f in FLAG_SETS[flags] for a in ("-Xarch_host", f)]


@functools.lru_cache(maxsize=None)
def _library():
    """-> (hipcc, the twelve instantiation objects of the library as built)"""
    from logreg_amd import build as b
    b.build(verbose=False)
    insts = [p for p in b.unit_objects() if os.path.basename(p).startswith("lr_inst_")]
    assert len(insts) == 12
    return b._hipcc(), insts


@functools.lru_cache(maxsize=None)
def shared_objects(flags):
    """-> (the stub, lr_api.hip, the twelve instantiation objects), the first two compiled under FLAG_SETS[flags]"""
    hipcc, insts = _library()
    if not os.path.exists(CXX):
        pytest.skip("ROCm's clang++ not found")
    stub, api = (os.path.join(_tmp(), f"{k}_{flags}.o") for k in ("stub", "api"))
    _do([CXX, *COMMON, *FLAG_SETS[flags], "-c", os.path.join(HOST, "hip_stub.cpp"), "-o", stub])
    _do([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *_xarch_host(flags), *INC, '-DLR_BUILD_ID="sanitizer-harness"', "-c",
         os.path.join(REPO, "logreg_amd", "csrc", "lr_api.hip"), "-o", api])
    return (stub, api, *insts)


@functools.lru_cache(maxsize=None)
def harness(source, flags="asan"):
    """tests/host/<source> compiled under FLAG_SETS[flags] and linked against shared_objects(flags) -> the executable"""
    stub, *rest = shared_objects(flags)
    stem = os.path.splitext(source)[0]
    obj, exe = os.path.join(_tmp(), f"{stem}_{flags}.o"), os.path.join(_tmp(), f"{stem}_{flags}")
    _do([CXX, *COMMON, *FLAG_SETS[flags], "-c", os.path.join(HOST, source), "-o", obj])
    _do([CXX, *FLAG_SETS[flags], stub, obj, *rest, "-ldl", "-lpthread", "-o", exe])  # (the stub first: its books exist before a code object registers)
    return exe


def run(exe, *args, timeout=600):
    """Run a harness; no sanitizer report, exit status 0 and a summary line of 0 failures, or the test fails -> the completed process"""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **RUN_ENV))
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert not any(s in r.stderr for s in REPORTS), tail
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures"), tail
    return r


def last_line(r):
    return r.stdout.strip().splitlines()[-1]


@functools.lru_cache(maxsize=None)
def plan_harness():
    """tests/host/plan_harness.hip: the library's planning code as a host program (no HIP call, so no stub), host side under
    AddressSanitizer + UBSan (a finding aborts the harness and fails the test) -> the executable"""
    hipcc, insts = _library()
    obj, exe = os.path.join(_tmp(), "plan_harness.o"), os.path.join(_tmp(), "plan_harness")
    _do([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *_xarch_host("asan"), *INC, "-c", os.path.join(HOST, "plan_harness.hip"), "-o", obj])
    _do([hipcc, "--offload-arch=gfx950", *_xarch_host("asan")[:2], obj, *insts, "-o", exe])
    return exe
