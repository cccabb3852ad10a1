"""The HOST ENGINE of liblogreg_hip.so under the sanitizers, in the GPU-less container (SURVEY section 5 "sanitizers").

lr_api.hip / lr_engine.h / lr_model.h / lr_plan.h -- the 1 200 lines that own model handles, device images, workspaces, per-stream
side slots, the fork / join events of two-part plans and every argument check -- are compiled with -fsanitize=address,undefined (and,
separately, -fsanitize=thread) and linked, with the library's own instantiation objects, against tests/host/hip_stub.cpp: the 31 HIP
runtime calls the library makes, on the host heap, launches as validated no-ops.  tests/host/engine_harness.cpp then drives the C ABI:
13 model shapes x 2 dtypes (every image kind) x all four kernel families x both precision policies, host and device buffers,
statistics, planned shards, the Hessian, every forced (mode, group), lr_run_nuts beside them everywhere (host and device buffers, with
and without samples, counters, depths and statistics; refused exactly where lr_plan_run refuses it), two chain sets on two streams + a
wide model on alternating streams, 60 error returns, a failing device allocation at EVERY allocation of model creation and of a run
(LR_ERR_NOMEM, nothing leaked, the model still usable), at every array the host-pointer path of a run, of lr_run_nuts and of lr_eval
stages (one device buffer per array given, none for one left out; LR_ERR_NOMEM, nothing leaked, the same call works next), and a model, its stream, buffers and runs on device 1 of two (what a rank > 0 of the multi-GPU job does:
not one allocation, creation or launch may happen with device 0 current, none may touch another device's stream or event), and the four
accumulators of kept draws with lr_psis (csrc/lr_accum.h: their whole life from host and device buffers in both dtypes, padded and not,
host input one item longer than a staging piece, every refused argument, a failing allocation at every allocation of create,
accumulate and result: LR_ERR_NOMEM, the count unchanged, nothing leaked, usable afterwards).  A sanitizer report, a leak, a wait on an unrecorded event or a bad launch configuration fails the test.
(First run, round 6: found that a failed hipMalloc left HIP's sticky error for the next launch check to trip over -- lr_model.h fail().)"""
import host_build


def test_host_engine_under_asan_and_ubsan():
    last = host_build.last_line(host_build.run(host_build.harness("engine_harness.cpp", "asan"), "all"))
    assert last.startswith("engine harness (all):"), last
    launches = int(last.split(":")[1].split("kernel launches")[0])
    assert launches > 3000  # (every engine did launch: chain kernels, the tall and the wide stepwise kernels)
    for fam in ("k_chain*", "k_tall*", "k_wide*"):
        assert int(last.split(fam)[0].split()[-1].strip("(,")) > 100, last


def test_host_engine_two_threads_under_tsan():
    """Two host threads on DIFFERENT handles (a float32 model with two-part launches on its own stream; a float64 wide model on the
    stepwise engine on another): the library's only shared state is per-thread (the error message) or per-handle."""
    host_build.run(host_build.harness("engine_harness.cpp", "tsan"), "threads")
