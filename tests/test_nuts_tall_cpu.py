"""NUTS on the stepwise engine (logreg_amd/csrc/lr_tall_nuts.h, lr_nuts_sched.h) in the GPU-less container: the planner through
tests/host/plan_harness.hip (the library's own planning code as a host program), the launch schedule and the workspace carve through
tests/host/nuts_sched_harness.cpp (a program with its own main under AddressSanitizer + UBSan), and the reference alone over the cases
of the GPU test, which may leave out a transition only below a reference margin the reference itself almost never falls under."""
import os
import subprocess

import pytest

from conftest import REPO
import nuts_reference as nr
import nuts_tall_cases as tc
from test_planner_cpu import harness  # noqa: F401  (the fixture: plan_harness.hip built as that module builds it)

NUTS, NUTS_DENSE, HMC = 4, 5, 2  # `kind` as plan_harness.hip passes it to plan_run (LR_KIND_NUTS, lr_plan.h kKindNutsDense)
AUTO, STEPWISE = -1, 4


def ask_kind(harness, requests, cus=256):  # noqa: F811
    """plan requests with a numeric kind: (dtype, p, n, chains, kind, group, mode) -> plan dicts or ("ERR", text)"""
    text = "".join(f"{d} {p} {n} {c} {k} 1 {g} {m} {cus}\n" for d, p, n, c, k, g, m in requests)
    r = subprocess.run([harness.exe], input=text, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    res = []
    for line in r.stdout.strip().split("\n"):
        f = line.split()
        res.append(("ERR", line) if f[0] == "ERR" else {"mode": int(f[0]), "group": int(f[1]), "rows": int(f[2]), "split": int(f[7])})
    return res


SHAPES = [(100000, 8), (20000, 8), (100, 40), (4096, 128)]


def test_stepwise_mode_plans_nuts_on_the_stepwise_engine(harness):  # noqa: F811
    for dtype in (0, 1):
        reqs = [(dtype, p, n, 1024, NUTS, 0, STEPWISE) for n, p in SHAPES]
        hmc = ask_kind(harness, [(dtype, p, n, 1024, HMC, 0, STEPWISE) for n, p in SHAPES])
        for (n, p), pl, ph in zip(SHAPES, ask_kind(harness, reqs), hmc):
            assert not isinstance(pl, tuple), (n, p, pl)
            assert pl["mode"] == STEPWISE and pl["split"] == 0, (n, p, pl)
            # group = row slices of `rows` rows: they cover the data, the last one is not empty, and there are no more than
            # check_group_for admits (one per 32-row block)
            assert pl["group"] * pl["rows"] >= n > (pl["group"] - 1) * pl["rows"], (n, p, pl)
            assert 1 <= pl["group"] <= (n + 31) // 32, (n, p, pl)
            assert (pl["group"], pl["rows"]) == (ph["group"], ph["rows"]), (pl, ph)  # the stepwise plan of the engine's other samplers


def test_an_explicit_slice_count_is_honoured(harness):  # noqa: F811
    res = ask_kind(harness, [(0, 8, 100000, 1024, NUTS, 40, STEPWISE), (1, 8, 20000, 64, NUTS, 7, STEPWISE), (0, 128, 4096, 1024, NUTS, 8, STEPWISE),
                             (1, 40, 100, 8, NUTS, 2, STEPWISE), (0, 8, 20000, 64, NUTS, 10 ** 6, STEPWISE)])
    assert [r["group"] for r in res[:4]] == [40, 7, 8, 2], res
    assert all(r["mode"] == STEPWISE for r in res[:4])
    assert res[4][0] == "ERR" and "exceeds" in res[4][1]


def test_automatic_mode_still_refuses_and_says_how(harness):  # noqa: F811
    res = ask_kind(harness, [(0, p, n, 1024, NUTS, 0, AUTO) for n, p in SHAPES])
    assert all(r[0] == "ERR" for r in res), res
    assert "beyond" in res[0][1] and "beyond" in res[1][1] and "p = 40 > 32" in res[2][1] and "p = 128 > 32" in res[3][1]
    assert all("LR_MODE_STEPWISE" in r[1] for r in res), res
    small = ask_kind(harness, [(0, 8, 200, 1024, NUTS, 0, AUTO)])[0]
    assert (small["mode"], small["group"]) == (1, 16)  # rows in LDS on 16 lanes per chain, as before


def test_the_dense_metric_is_refused_on_the_stepwise_engine(harness):  # noqa: F811
    res = ask_kind(harness, [(0, 8, 200, 64, NUTS_DENSE, 0, STEPWISE), (0, 8, 100000, 64, NUTS_DENSE, 0, STEPWISE), (0, 40, 100, 64, NUTS_DENSE, 0, STEPWISE),
                             (0, 40, 100, 64, NUTS_DENSE, 0, AUTO), (0, 8, 100000, 64, NUTS_DENSE, 0, AUTO)])
    assert all(r[0] == "ERR" for r in res), res
    assert "stepwise (tall-data) engine has no NUTS kernel" in res[0][1] and "stepwise (tall-data) engine has no NUTS kernel" in res[1][1]
    assert not any("LR_MODE_STEPWISE" in r[1] for r in res), res  # no hint at a path the dense metric does not have


def test_launch_schedule_and_workspace_carve_under_the_sanitizers(tmp_path):
    """(d, i) equal nuts_run's recurrence for every step up to 1023, the host reads only at s = 2^(d+1) - 2, a tally that never
    reaches zero ends after 2^max_depth - 1 steps, the carve sizes for P = 4 .. 128 (tests/host/nuts_sched_harness.cpp)."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "c++"
    exe = str(tmp_path / "nuts_sched_harness")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "logreg_amd", "csrc"),
                        os.path.join(REPO, "tests", "host", "nuts_sched_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("nuts_sched:") and last.endswith(" 0 failures") and int(last.split()[1]) > 10000, tail


@pytest.fixture(scope="module")
def reference_alone():
    return [(c, tc.reference_free_running(c)) for c in tc.F64_CASES + [tc.OFF_CHIP]]


def test_the_reference_stays_within_the_margin_cap_of_the_gpu_test(reference_alone):
    """The GPU test leaves a transition out below nr.MIN_MARGIN and allows 1 in 1000: the reference, free-running over the same cases,
    must itself stay within that."""
    n = sum(len(res) for _, res in reference_alone)
    low = [(c, t.reason, t.margin) for c, res in reference_alone for t in res if not t.margin >= nr.MIN_MARGIN and not any(x != x for x in t.x)]
    print(f"{n} reference transitions, {len(low)} below the margin {nr.MIN_MARGIN:g}")
    assert n > 2000 and len(low) < n / 1000, low[:5]


def test_the_cases_reach_what_the_gpu_test_asserts(reference_alone):
    """every padded width beyond depth 7, every stop reason, the chain counts and shapes the kernel's paths need"""
    import collections
    cnt, deep = collections.Counter(), collections.Counter()
    for c, res in reference_alone:
        for t in res:
            cnt[t.reason] += 1
            deep[tc.padded(c.case.p)] += abs(t.depth) >= 7
    assert all(deep[P] >= 3 for P in (4, 8, 16, 32, 64, 128)), dict(deep)
    assert all(cnt[r] >= 20 for r in (nr.DIVERGENCE, nr.SUBTREE, nr.TREE, nr.MAX_DEPTH)), dict(cnt)
    cases = [c.case for c in tc.F64_CASES]
    assert {3, 8, 17, 32, 33, 64, 65, 128} <= {c.p for c in cases} and {c.C for c in cases} == {1, 3, 8, 9, 65, 257}
    assert {c.max_depth for c in cases} == {1, 2, 6, 10} and any(c.iter_offset >= 2 ** 32 for c in cases)
    assert {g.group for g in tc.F64_CASES if g.case.p <= 32} == {0, 1, 3, 4}


def test_every_narrow_case_is_a_shape_the_stepwise_mode_accepts(harness):  # noqa: F811
    reqs = [(1, g.case.p, g.case.n, g.case.C, NUTS, g.group, STEPWISE) for g in tc.F64_CASES + [tc.OFF_CHIP]]
    reqs += [(0, g.case.p, g.case.n, g.case.C, NUTS, g.group, STEPWISE) for g in tc.F32_NARROW + tc.F32_WIDE]
    for rq, pl in zip(reqs, ask_kind(harness, reqs)):
        assert not isinstance(pl, tuple) and pl["mode"] == STEPWISE, (rq, pl)
    asked = [(rq, pl) for rq, pl in zip(reqs, ask_kind(harness, reqs)) if rq[5] > 1]
    assert asked and all(pl["group"] == rq[5] and rq[2] % pl["rows"] != 0 for rq, pl in asked), asked  # asked slices, a shorter last one


def test_shapes_the_fused_kernel_takes_keep_refusing_the_stepwise_mode(harness):  # noqa: F811
    """what ran or was refused before is unchanged: rows that fit the LDS run fused, and LR_MODE_STEPWISE is refused for them"""
    res = ask_kind(harness, [(0, 8, 200, 300, NUTS, 0, STEPWISE), (1, 8, 200, 300, NUTS, 2, STEPWISE), (0, 4, 64, 64, NUTS, 0, STEPWISE),
                             (1, 32, 250, 64, NUTS, 0, STEPWISE), (0, 8, 4000, 64, NUTS, 0, STEPWISE)])
    assert all(r[0] == "ERR" and "rows in LDS" in r[1] for r in res), res
