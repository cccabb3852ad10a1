"""The launches of the stepwise engine, pinned in the GPU-less container: which kernel, with which grid, block and LDS, on which
stream, in which order.  tests/host/engine_harness.cpp `trace` runs the C ABI on the stub HIP runtime (tests/host/hip_stub.cpp) over
the shapes on both sides of every rule of lr_plan.h plan_stepwise x L = 1, 2, 3, 4, 8 x the three precision policies x the debug
options, the other kernel families, lr_eval, NUTS and a planned shard, and prints each case's launches.  The expectation,
tests/golden/stepwise_launch_trace.txt, was recorded with the same stub and harness from the engine of the commit its first line names --
the launch loop before it was rewritten to state every launch on an argument block it never edits.

The trace does not see a launch's arguments (part_f32, fuse_mid, which buffer of a pair is read): tests/test_gpu_stepwise_parent.py
compares the bytes that come out."""
import difflib
import os

from conftest import REPO
import host_build


def test_stepwise_launch_sequence_is_the_recorded_one():
    r = host_build.run(host_build.harness("engine_harness.cpp", "plain"), "trace")
    with open(os.path.join(REPO, "tests", "golden", "stepwise_launch_trace.txt")) as f:
        want = f.read().split("\n", 1)[1]  # (the first line names the commit the trace was recorded from)
    got = r.stdout
    assert got == want, "".join(list(difflib.unified_diff(want.splitlines(True), got.splitlines(True), "recorded", "this tree", n=1))[:60])
    assert got.count("\n== ") + 1 >= 19 * 3 and "k_wide_traj2_bf16" in got and "k_tall_partial_mx16" in got and "k_tall_nuts_update" in got
