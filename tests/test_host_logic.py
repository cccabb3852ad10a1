"""Host-side logic that needs no GPU: diagnostics, data loader, the generic (reference-semantics)
kernel constructors driven by oracle closures, chunk planning, sharding arithmetic."""
import numpy as np
import pytest

from conftest import REPO, load_golden
import logreg_amd as la
from logreg_amd import kernels as K
from logreg_amd.distributed import shard_bounds

PRE = np.array([100.0, 1, 1, 1, 1, 1, 25, 1])


def test_loader_reproduces_reference_data_block(pima):
    X, y = la.load_pima()
    Xg, yg = pima
    assert X.shape == (200, 8) and np.array_equal(X, Xg) and np.array_equal(y, yg)
    assert y.sum() == 68 and np.all(X[:, 0] == 1)
    assert X[:, 1:].max(axis=0).tolist() == [14, 199, 110, 99, 47.9, 2.288, 63]


def test_loader_rejects_malformed_rows(tmp_path):
    p = tmp_path / "bad.data"
    p.write_text("1 2 3 4 5 6 7 Maybe\n")
    with pytest.raises(ValueError):
        la.load_pima(str(p))


def test_ess_on_ar1_process():
    rng = np.random.default_rng(0)
    n, phi = 200000, 0.8
    e = rng.standard_normal(n)
    x = np.empty(n)
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    ess = la.ess_geyer(x)
    assert ess == pytest.approx(n * (1 - phi) / (1 + phi), rel=0.1)
    assert la.ess_geyer(rng.standard_normal(5000)) == pytest.approx(5000, rel=0.15)


def test_ess_matches_reference_fixture_scale():
    # the F7 fixture's ESS was produced with this estimator on the reference's own output
    g = load_golden("posterior_hmc.json")
    for run in g["runs"]:
        ess = np.array(run["ess"])
        assert ess.shape == (8,) and np.all(ess > 2000) and np.all(ess <= 10000)
        assert np.argmin(ess) == 0  # b0 mixes slowest, as BASELINE.md reports


def test_summarise_and_describe_shapes():
    rng = np.random.default_rng(1)
    s = rng.standard_normal((500, 16, 3)) * np.array([1.0, 2.0, 3.0])
    summ = la.summarise(s)
    assert np.allclose(summ["sd"], [1, 2, 3], rtol=0.05)
    assert np.all(summ["ess"] > 0.6 * 500 * 16)
    d = la.describe(s)
    assert d["nobs"] == 8000 and np.allclose(d["variance"], [1, 4, 9], rtol=0.1)


@pytest.mark.parametrize("kind", ["hmc", "mala", "rwmh", "ul"])
def test_generic_kernels_have_reference_semantics(oracle_model, kind):
    """mhKernel/malaKernel/hmcKernel/ulKernel/mcmc with arbitrary callables (here: the oracle's
    closures) consume NumPy's global RNG exactly like the reference, so re-seeding as the
    fixture generator did replays the reference's recorded chain (F6)."""
    g = load_golden("accept_replay.json")
    rec, par = g[kind], g["params"][kind]
    lpost, glp = oracle_model.lpost, oracle_model.glp
    if kind == "hmc":
        k = la.hmcKernel(lpost, glp, eps=par["eps"], l=par["l"], dmm=np.array(par["dmm"]))
    elif kind == "mala":
        k = la.malaKernel(lpost, glp, dt=par["dt"], pre=np.array(par["pre"]))
    elif kind == "ul":
        k = la.ulKernel(glp, dt=par["dt"], pre=np.array(par["pre"]))
    else:
        sd = np.array(par["prop_sd"])
        k = la.mhKernel(lpost, lambda b: b + sd * np.random.randn(8))
    assert not isinstance(k, la.FusedKernel)
    steps = 40
    np.random.seed(1000 + len(kind))
    out = la.mcmc(np.array(rec["init"]), k, thin=1, iters=steps, verb=False)
    np.testing.assert_allclose(out, np.array(rec["states"])[:steps], rtol=1e-6, atol=1e-9)
    # thin semantics
    np.random.seed(1000 + len(kind))
    out4 = la.mcmc(np.array(rec["init"]), k, thin=4, iters=steps // 4, verb=False)
    np.testing.assert_allclose(out4, np.array(rec["states"])[3:steps:4], rtol=1e-6, atol=1e-9)


def test_mcmc_prints_like_the_reference(oracle_model, capsys):
    k = la.ulKernel(oracle_model.glp, dt=1e-6, pre=PRE)
    la.mcmc(np.zeros(8), k, thin=1, iters=3)
    out = capsys.readouterr().out
    assert out == "3 iterations\n0 1 2 \nDone.\n"


def test_auto_chunk_bounds_launch_length():
    class M:
        n, p = 200, 8
    k = K.FusedKernel.__new__(K.FusedKernel)
    k.kind, k.params, k.model = "hmc", {"l": 50}, M()
    c = K._auto_chunk(k, 4096, 20, 10000)
    assert 1 <= c <= 10000 and c * 20 * 50 * 1600 <= 2_000_000_000
    M.n = 100000
    assert K._auto_chunk(k, 1024, 20, 10000) == 2
    k.kind = "rwmh"
    assert K._auto_chunk(k, 1, 1000, 10000) == 2


def test_shard_bounds_partition():
    for C, W in ((65536, 8), (10, 3), (7, 8), (4096, 1)):
        b = [shard_bounds(C, W, r) for r in range(W)]
        assert b[0][0] == 0 and b[-1][1] == C
        assert all(b[i][1] == b[i + 1][0] for i in range(W - 1))
        sizes = [hi - lo for lo, hi in b]
        assert max(sizes) - min(sizes) <= 1


def test_synthetic_design_is_deterministic():
    X1, y1, b1 = la.synthetic_logreg(200, 8)
    X2, y2, b2 = la.synthetic_logreg(200, 8)
    assert np.array_equal(X1, X2) and np.array_equal(y1, y2) and np.all(X1[:, 0] == 1)
    assert set(np.unique(y1)) <= {0.0, 1.0}


def test_output_writer_roundtrip(tmp_path):
    pd = pytest.importorskip("pandas")
    pytest.importorskip("pyarrow")
    rng = np.random.default_rng(0)
    one = rng.standard_normal((50, 8))
    path = la.write_parquet(one, str(tmp_path / "fit.parquet"))
    df = pd.read_parquet(path)
    assert list(df.columns) == ["b0", "b1", "b2", "b3", "b4", "b5", "b6", "b7"]  # fit-np-hmc.py:111
    np.testing.assert_array_equal(la.read_parquet(path), one)
    many = rng.standard_normal((20, 3, 8)).astype(np.float32)
    path = la.write_parquet(many, str(tmp_path / "many.parquet"))
    np.testing.assert_array_equal(la.read_parquet(path), many)
    d = la.print_summary(one)
    assert d["nobs"] == 50


def test_find_map_on_oracle_closures(oracle_model, map_beta, pscale):
    """The Newton warm start only needs an object with .p and .hessian(beta) -> (lpost, glp, H)."""
    class Shim:
        p = 8

        def hessian(self, beta):
            X, y = oracle_model.X, oracle_model.y
            mu = 1.0 / (1.0 + np.exp(-X @ beta))
            H = (X * (mu * (1 - mu))[:, None]).T @ X + np.diag(1.0 / pscale ** 2)
            return oracle_model.lpost(beta), oracle_model.glp(beta), H
    from logreg_amd.optimize import find_map
    beta, info = find_map(Shim(), np.zeros(8))
    assert info["converged"] and info["iterations"] < 15
    assert oracle_model.lpost(beta) == pytest.approx(-100.44943693563212, abs=1e-9)
    np.testing.assert_allclose(beta, map_beta, atol=2e-5)  # BFGS itself stopped at |glp| ~ 7e-7
    assert np.max(np.abs(info["grad"])) < 1e-6


def test_split_rhat_and_overdispersed_init():
    rng = np.random.default_rng(3)
    good = rng.standard_normal((400, 8, 3))
    assert np.all(np.abs(la.split_rhat(good) - 1.0) < 0.02)
    bad = good + np.arange(8)[None, :, None]  # chains stuck at different levels
    assert np.all(la.split_rhat(bad) > 1.5)
    init = la.overdispersed_init(np.zeros(3), np.array([1.0, 2.0, 3.0]), 5000, scale=2.0, seed=1)
    assert init.shape == (5000, 3)
    np.testing.assert_allclose(init.std(axis=0), [2.0, 4.0, 6.0], rtol=0.05)
    np.testing.assert_array_equal(init, la.overdispersed_init(np.zeros(3), np.array([1.0, 2.0, 3.0]), 5000, 2.0, 1))


@pytest.mark.parametrize("world", [2, 8])
def test_bench_launch_plumbing_under_torchrun_gloo(world):
    """bench.py as the driver launches it for N > 1 (`python -m torch.distributed.run --nproc-per-node N ... bench.py
    --gpus N ...`), N = 2 and the full node's 8: `--dry-run` runs bench.py's own Exchange object -- the one the GPU run
    uses -- on the gloo backend with a CPU tensor for the sample buffer, so rank/world parsing, weak-scaling chain offsets
    (0 ... 7 x 4096), the gather to rank 0 (shapes and contents), the barrier and the max / sum reductions run here."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), __import__("os").path.join(REPO, "bench.py"),
                        "--gpus", str(world), "--steps", "3", "--warmup", "1", "--dry-run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["chain_offsets"] == [4096 * r for r in range(world)] and d["scaling"] == "weak"
    assert d["gather_ok"] and d["sum_over_ranks_ok"] and d["gather_ms"] > 0 and d["wall_ms"] >= d["gather_ms"]
    # the self-check block of an N > 1 line (bench.self_check, the code the GPU run executes)
    assert d["ranks_seen"] == world and len(d["devices"]) == world and d["devices_distinct"]
    assert d["kernel_ms_min"] == pytest.approx(0.1) and d["kernel_ms_max"] == pytest.approx(0.1 * world)
    assert d["gather_bitexact"] is True and d["gather_checked_rank"] == 1 and d["gather_checked_chains"] == 64


def _torchrun(world, script, *args, timeout=900):
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), script, *args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 8])
def test_bench_multi_gpu_line_on_the_abi_test_double(world):
    """bench.py's REAL main() at N > 1 -- the product's ChainSets with global chain ids, the gather inside the timed region,
    the self-check block (ranks seen, device identities, kernel time min / max, rank 0 re-running 64 chains of rank 1's block and
    comparing them bit for bit with what the gather delivered) and BASELINE configs 3 and 5 across the ranks (MALA with the
    gather AND with the summary all-reduce; wide-model HMC with the gather) -- under torch.distributed.run on gloo, the C ABI
    being the CPU test double (tests/bench_on_twin.py injects it; chain counts scaled down 64x, marked in the rows)."""
    import os
    d = _torchrun(world, os.path.join(REPO, "tests", "bench_on_twin.py"), "--gpus", str(world), "--chains", "80", "--steps", "2",
                  "--warmup", "1", "--prewarm", "0.02", "--scale", "64", "--full")
    assert d["n_gpus"] == world and d["config"]["chains_per_gpu"] == 80 and d["value"] > 0 and d["gather_ms"] > 0
    mg = d["multi_gpu"]
    assert mg["ranks_seen"] == world and len(mg["devices"]) == world and mg["devices_distinct"]
    assert 0 < mg["kernel_ms_min"] <= mg["kernel_ms_max"]
    assert mg["gather_bitexact"] is True and mg["gather_checked_rank"] == 1 and mg["gather_checked_chains"] == 64
    # north_star: "chains/sec and achieved-HBM-fraction reported at 1/2/4/8 GPUs" -- one row per rank from the rank's own event time,
    # and the weak-scaling row of the headline (fixed chains per GPU)
    assert len(mg["kernel_ms_per_rank"]) == world and min(mg["kernel_ms_per_rank"]) == pytest.approx(mg["kernel_ms_min"], rel=1e-3)
    per = d["per_rank"]
    assert [r["rank"] for r in per] == list(range(world))
    for r in per:
        assert r["chain_iterations_per_s"] == pytest.approx(80 * 20 / (r["kernel_ms"] / 1e3), rel=1e-9)
        assert r["grad_evals_per_s"] == pytest.approx(50 * r["chain_iterations_per_s"]) and 0 < r["hbm_frac"] < 1 and r["valu_frac"] > 0
    ws = d["weak_scaling"]
    assert ws["chains_per_gpu"] == 80 and ws["n_gpus"] == world and ws["chains_total"] == 80 * world
    assert ws["chain_iterations_per_s"] == d["value"] and ws["per_gpu"] == pytest.approx(d["value"] / world) and 0 <= ws["gather_share"] < 1
    rows = {r["config"]: r for r in d["extra"]["configs"]}
    assert set(rows) == {3, 5} and all(r["n_gpus"] == world and r["scaled_down"] == 64 for r in rows.values())
    c3, c5 = rows[3], rows[5]
    assert c3["chains_total"] == world * 128 and c3["with_gather"]["blocks_ok"] and c3["with_gather"]["gather_ms"] > 0
    assert c3["summary_only"]["chains_counted"] == world * 128 and c3["summary_only"]["doubles_per_rank"] == 57
    assert c3["summary_only"]["allreduce_ms"] > 0 and c3["roofline"]["frac"] > 0
    assert c5["chains_total"] == world * 16 and c5["blocks_ok"] and 0.3 < c5["accept_rate"] <= 1.0 and c5["roofline"]["bound"] == "mfma"
    assert c5["gathered_bytes_per_rank"] == 16 * 128 * 4


def test_bench_gpus_n_without_a_launcher_starts_its_own_ranks():
    """The driver's N > 1 invocation may be a PLAIN `python bench.py --gpus N ...` (BENCH_r04.json.cmd): with no WORLD_SIZE in
    the environment bench.main() must start the N ranks itself (a torch.distributed.run child, before any GPU call) and relay
    rank 0's one line and the exit code -- never measure one GPU silently.  Here: the real main() on the ABI test double over
    gloo, world 2, launched as a plain process."""
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "bench_on_twin.py"), "--gpus", "2", "--chains", "80", "--steps", "2",
                        "--warmup", "1", "--prewarm", "0.02", "--scale", "64", "--full"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "without a launcher: starting 2 ranks" in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["multi_gpu"]["ranks_seen"] == 2 and d["multi_gpu"]["gather_bitexact"] is True
    assert {row["config"] for row in d["extra"]["configs"]} == {3, 5}



def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_whatever_the_prewarm(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` (the real main() on the ABI test double) times N steps and prints the headline
    line without the --full measurements; --dump-outputs writes the last timed step's kept samples.  The pre-warm runs on chains of
    its own, so two runs whose time-bounded pre-warms differ (none, and one batch of 20 launches) dump identical samples."""
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines, dumps = [], []
    for i, prewarm in enumerate(("0", "0.001")):
        out = tmp_path / f"dump{i}"
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "bench_on_twin.py"), "--gpus", "1", "--chains", "16", "--steps", "3",
                            "--warmup", "1", "--prewarm", prewarm, "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        lines.append(json.loads(js[0]))
        assert sorted(os.listdir(out)) == ["samples.npy"]
        dumps.append(np.load(out / "samples.npy"))
    assert [d["prewarm"]["steps"] for d in lines] == [0, 20]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "chain-iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["value"] == pytest.approx(16 * 3 * 20 / (3 * d["ms_per_step"] / 1e3), rel=1e-9)
        assert not {"extra", "ess", "min_ess_per_s", "cpu_baseline", "reference_arithmetic", "host_boundary"} & set(d)
    assert dumps[0].shape == (16, 8) and dumps[0].dtype == np.float32 and np.isfinite(dumps[0]).all()
    assert np.array_equal(dumps[0], dumps[1])

def test_bench_refuses_more_ranks_than_gpus():
    """`--gpus 2` over RCCL on a node with fewer than 2 GPUs (this container has none): the ranks refuse before the rendezvous
    and the plain invocation exits non-zero -- it does not fall back to one GPU."""
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=env)
    import torch
    if torch.cuda.device_count() < 2:
        assert r.returncode != 0
        assert "refusing to share GPUs" in r.stderr
        assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_self_check_detects_a_wrong_block():
    """gather_bitexact is a real comparison: a re-run that differs in one element, or a gather that delivered the blocks in
    another order, reads false."""
    import sys
    import torch
    sys.path.insert(0, REPO)
    import bench
    ex = bench.Exchange("gloo", 0, 1, 0)  # no process group: reductions are identities
    blocks = [torch.arange(3 * 70 * 8, dtype=torch.float32).reshape(3, 70, 8) + 1000 * r for r in range(2)]
    good = bench.self_check(ex, "pci=a", 0.5, blocks, 1, lambda r: blocks[r][:, :64].numpy().copy())
    assert good["gather_bitexact"] is True and good["ranks_seen"] == 1 and good["kernel_ms_min"] == good["kernel_ms_max"] == 0.5
    off = blocks[1][:, :64].numpy().copy()
    off[2, 63, 7] = np.nextafter(off[2, 63, 7], np.float32(np.inf))
    assert bench.self_check(ex, "pci=a", 0.5, blocks, 1, lambda r: off)["gather_bitexact"] is False
    assert bench.self_check(ex, "pci=a", 0.5, blocks[::-1], 1, lambda r: blocks[r][:, :64].numpy())["gather_bitexact"] is False
