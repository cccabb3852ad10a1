"""Cases and fixture generator of tests/test_gpu_nuts_host_parent.py: everything the host puts between the C ABI and the four NUTS kernel
instantiations (diagonal or dense metric, fixed or tuned) -- argument packing, the metric triples, the launch table, the warm-up handle --
at the smallest shapes where the padded widths and the chain tilings differ.  Results are compared BYTE FOR BYTE with a recording made
on another build:

    python tests/nuts_host_cases.py --write tests/golden/nuts_host_parent.json --commit <id of the recorded build's commit>

run once, on the GPU, in a checkout of that commit (this file copied into its tests/).  Every array is recorded as the SHA-256 of its
bytes (equal digests = equal bytes); arrays of runs of up to 5 chains are recorded in full as hex as well, so that a difference can be read,
where the array has at most 1024 bytes: with the warm-ups' draws and traces in full the file was 900 KB, more than a fixture should weigh.
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(REPO, "tests", "golden", "nuts_host_parent.json")
SEED, OFFSET = 20263, 7  # Philox key; chain_offset: not a multiple of 4
FULL_HEX_CHAINS, FULL_HEX_BYTES = 5, 1024
N = 50
# p = 3, 8, 20 are padded to 4, 8, 32: the small-gather path, one 16-lane slice and two
MODELS = [(p, dtype) for p in (3, 8, 20) for dtype in ("float32", "float64")]
METRICS = ("diag", "dense")
MAX_DEPTH = 4
RUN_CHAINS = (1, 5, 257)  # one chain, a partial wave, a workgroup and a tail
RUN_THIN, RUN_KEPT, RUN_EPS = 2, 3, 0.2
WARM_CHAINS = (5, 257)
WARM_W = 40               # one window, [.., 36): a window end, a dual-averaging restart, one dense re-factorisation, the final iteration
WARM_ADAPT = (True, False)
COUNTERS = ("n_leapfrog", "divergent", "max_depth_hits", "mean_depth", "mean_accept_stat")


def data(p):
    """A small synthetic logistic regression, from NumPy's PCG64 streams only."""
    rng = np.random.default_rng(1000 * N + p)
    X = rng.standard_normal((N, p))
    X[:, 0] = 1.0
    beta = rng.standard_normal(p) * 0.5
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return X, y, np.linspace(1.0, 3.0, p)  # a different prior scale per coordinate: a coordinate that lands in the wrong lane shows


def dmm(p):
    return np.linspace(0.5, 2.0, p)


def inv_metric(p):
    """SPD: diag(1 / dmm) scaled on both sides around 0.8 I + 0.2 R with R_ij = 0.5^|i - j| (a correlation matrix)"""
    s = np.sqrt(1.0 / dmm(p))
    i = np.arange(p)
    return (0.8 * np.eye(p) + 0.2 * 0.5 ** np.abs(i[:, None] - i[None, :])) * np.outer(s, s)


def init(p, C):
    return 0.3 * np.random.default_rng(31 * p + C).standard_normal((C, p))


def record(arrays, C):
    rec = {}
    for name, arr in arrays.items():
        arr = np.ascontiguousarray(arr)
        rec[name] = {"dtype": str(arr.dtype), "shape": list(arr.shape), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}
        if C <= FULL_HEX_CHAINS and arr.nbytes <= FULL_HEX_BYTES:
            rec[name]["hex"] = arr.tobytes().hex()
    return rec


def run_fixed(la, p, dtype):
    """-> {case id: record} of lr_run_nuts and lr_run_nuts_dense on one model: kept samples, final state, counters, depths"""
    X, y, pscale = data(p)
    m = la.LogReg(X, y, pscale, dtype=dtype)
    res = {}
    try:
        for metric in METRICS:
            kw = {"dmm": dmm(p)} if metric == "diag" else {"inv_metric": inv_metric(p)}
            k = la.nutsKernel(m.lpost, m.glp, eps=RUN_EPS, max_depth=MAX_DEPTH, **kw)
            for C in RUN_CHAINS:
                cs = la.ChainSet(k, init(p, C), seed=SEED, chain_offset=OFFSET)
                depth = la.DeviceArray(m.device, (RUN_KEPT, C), np.int8)
                out = cs.advance(RUN_KEPT, RUN_THIN, depth=depth)
                cs.sync()
                res[f"run-{metric}-{dtype}-p{p}-C{C}"] = record({"samples": out.to_host(), "state": cs.state.to_host(),
                                                                 "counters": cs.get_counters(), "depth": depth.to_host()}, C)
    finally:
        m.close()
    return res


def run_warmup(la, p, dtype):
    """-> {case id: record} of nuts_warmup and nuts_warmup_dense on one model, with and without metric adaptation"""
    X, y, pscale = data(p)
    m = la.LogReg(X, y, pscale, dtype=dtype)
    res = {}
    try:
        for metric in METRICS:
            for adapt in WARM_ADAPT:
                for C in WARM_CHAINS:
                    kw = dict(num_warmup=WARM_W, eps=RUN_EPS, max_depth=MAX_DEPTH, adapt_metric=adapt, seed=SEED, chain_offset=OFFSET, keep=True)
                    if metric == "diag":
                        r = la.nuts_warmup(m.lpost, m.glp, init(p, C), dmm=dmm(p), **kw)
                        arrays = {"dmm": r.dmm}
                    else:
                        r = la.nuts_warmup_dense(m.lpost, m.glp, init(p, C), inv_metric=inv_metric(p), **kw)
                        arrays = {"inv_metric": r.inv_metric}
                    arrays.update({"eps": np.float64(r.eps), "trace": r.trace, "metric_trace": r.metric_trace, "state": r.state, "draws": r.draws})
                    arrays.update({f: r.info[f] for f in COUNTERS})
                    arrays["info"] = np.array([r.info[f] for f in ("metric_skipped", "windows", "iterations", "seed")], dtype=np.int64)
                    res[f"warmup-{metric}-{'metric' if adapt else 'step'}-{dtype}-p{p}-C{C}"] = record(arrays, C)
    finally:
        m.close()
    return res


def dump(doc, path):
    """the fixture as JSON with one array's record per line"""
    with open(path, "w") as f:
        f.write('{"recorded_from_commit": %s,\n"library_build_id": %s,\n"cases": {\n' % (json.dumps(doc["recorded_from_commit"]), json.dumps(doc["library_build_id"])))
        cases = sorted(doc["cases"].items())
        for i, (cid, rec) in enumerate(cases):
            rows = ",\n".join(f"{json.dumps(name)}: {json.dumps(r, sort_keys=True)}" for name, r in sorted(rec.items()))
            f.write("%s: {\n%s}%s\n" % (json.dumps(cid), rows, "," if i + 1 < len(cases) else ""))
        f.write("}}\n")


def case_ids():
    ids = {f"run-{metric}-{dtype}-p{p}-C{C}" for p, dtype in MODELS for metric in METRICS for C in RUN_CHAINS}
    return ids | {f"warmup-{metric}-{a}-{dtype}-p{p}-C{C}" for p, dtype in MODELS for metric in METRICS for a in ("metric", "step")
                  for C in WARM_CHAINS}


def run_all(la):
    res = {}
    for p, dtype in MODELS:
        res.update(run_fixed(la, p, dtype))
        res.update(run_warmup(la, p, dtype))
    return res


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True)
    ap.add_argument("--commit", required=True, help="id of the commit whose build is being recorded")
    a = ap.parse_args()
    import logreg_amd
    from logreg_amd import build as lib_build
    doc = {"recorded_from_commit": a.commit, "library_build_id": lib_build.built_id(), "cases": run_all(logreg_amd)}
    os.makedirs(os.path.dirname(os.path.abspath(a.write)), exist_ok=True)
    dump(doc, a.write)
    print(f"{len(doc['cases'])} cases -> {a.write} ({os.path.getsize(a.write)} bytes)")
