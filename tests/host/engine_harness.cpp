// engine_harness.cpp -- TEST INFRASTRUCTURE: the host engine of liblogreg_hip.so (lr_api.hip, lr_engine.h, lr_model.h, lr_plan.h)
// driven through its own C ABI on the stub HIP runtime (tests/host/hip_stub.cpp), built with -fsanitize=address,undefined or
// -fsanitize=thread by tests/test_engine_sanitizers.py.  Kernels do not run (a launch is a validated no-op), so nothing here checks a
// number: it checks that every path of the host engine -- model images of every kind, one- and two-part plans with their fork / join
// events, the stepwise engines and their workspaces, two chain sets on two streams, statistics, the Hessian, every error return, a
// failing allocation at every point of model creation -- touches only memory it owns, frees what it allocates, and waits only on
// events it recorded.  lr_run_nuts goes wherever the other kernel families go (and is refused where lr_plan_run refuses it), and the staged
// host-pointer path of a run, of lr_run_nuts and of lr_eval survives a failing allocation at each of its arrays.  The four accumulators of kept draws (lr_predict, lr_acf, lr_marg, lr_loo) and lr_psis go through the same: their
// whole life from host and device buffers, input longer than one staging piece, every refused argument, a failing allocation at every
// allocation of create, accumulate and result.
//   engine_harness all        every scenario on one thread
//   engine_harness threads    two host threads, one model / stream / chain set each, running concurrently (ThreadSanitizer)
//   engine_harness trace      the launches of the stepwise engine, case by case, as text (tests/test_stepwise_trace_cpu.py compares it with
//                             tests/golden/stepwise_launch_trace.txt, recorded from the engine before its launch loop was rewritten)
#include "harness.h"
#include "logreg_hip_acf.h"
#include "logreg_hip_loo.h"
#include "logreg_hip_marginals.h"
#include "logreg_hip_nuts.h"
#include "logreg_hip_predict.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

static long g_deliberate_bad_waits = 0;  // (scenario_errors asks for the elapsed time of an event it never recorded)

struct Data {
    std::vector<double> X, y, sd;
    int64_t n;
    int p;
};
static Data make_data(int64_t n, int p, unsigned seed) {
    Data d;
    d.n = n; d.p = p;
    d.X.resize((size_t)n * p); d.y.resize(n); d.sd.assign(p, 2.0);
    unsigned long long s = seed * 2654435761ull + 12345;
    auto u = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    for (int64_t i = 0; i < n; ++i) {
        d.X[(size_t)i * p] = 1.0;
        for (int j = 1; j < p; ++j) d.X[(size_t)i * p + j] = 2.0 * u() - 1.0;
        d.y[i] = u() < 0.5 ? 0.0 : 1.0;
    }
    return d;
}
// NUTS on one model: host and device buffers, with and without samples, counters, depths and statistics.  A shape or a forced
// (mode, group) the family has no kernel for is refused by every call, as lr_plan_run refuses it.
static void run_nuts(lr_model* m, const Data& d, int64_t C, int dtype, void* stream, int mode, int group) {
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int D = LR_NUTS_MAX_DEPTH;  // (the depth lr_plan_run plans for: the two agree on what fits the LDS)
    lr_run_opts o{};
    o.n_chains = C; o.thin = 2; o.iters = 2; o.seed = 7; o.mode = mode; o.group = group;
    int32_t mo, go, ro;
    const int want = lr_plan_run(m, LR_KIND_NUTS, &o, &mo, &go, &ro) == LR_OK ? LR_OK : LR_ERR_UNSUPPORTED;
    std::vector<unsigned char> state((size_t)C * d.p * es, 0), out((size_t)2 * C * d.p * es);
    std::vector<lr_nuts_counters> cnt(C, lr_nuts_counters{});
    std::vector<int8_t> depth((size_t)2 * C);
    std::vector<double> vec(d.p, 1.0), hstats((size_t)2 * C * 2 * d.p, 0.0);
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, out.data(), cnt.data(), depth.data()) == want, "nuts host, every array (C=%lld)", (long long)C);
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, nullptr, nullptr, nullptr) == want, "nuts host, the state alone");
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, out.data(), nullptr, depth.data()) == want, "nuts host, no counters");
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, nullptr, cnt.data(), nullptr) == want, "nuts host, counters alone");
    o.stats = hstats.data(); o.stats_batch = 1; o.stats_first = 0; o.stats_slots = 2;
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, nullptr, cnt.data(), nullptr) == want, "nuts host, statistics and counters");
    o.iters = 0;
    EXPECT(lr_run_nuts(m, state.data(), 0.01, D, vec.data(), &o, out.data(), cnt.data(), depth.data()) == want, "nuts host, no iterations");
    o.iters = 2;
    Dev dstate((size_t)C * d.p * es), dout((size_t)2 * C * d.p * es), dcnt((size_t)C * sizeof(lr_nuts_counters)), ddepth((size_t)2 * C), dstats((size_t)2 * C * 2 * d.p * 8);
    EXPECT(dstate.p && dout.p && dcnt.p && ddepth.p && dstats.p, "device buffers");
    o.on_device = 1; o.stream = stream; o.stats = (double*)dstats.p;
    const long on0 = hipstub_launches_on(stream);
    EXPECT(lr_run_nuts(m, dstate.p, 0.01, D, vec.data(), &o, dout.p, (lr_nuts_counters*)dcnt.p, (int8_t*)ddepth.p) == want, "nuts device, every array + statistics");
    o.stats = nullptr;
    EXPECT(lr_run_nuts(m, dstate.p, 0.01, D, vec.data(), &o, nullptr, nullptr, nullptr) == want, "nuts device, the state alone");
    EXPECT(lr_run_nuts(m, dstate.p, 0.01, D, vec.data(), &o, nullptr, (lr_nuts_counters*)dcnt.p, (int8_t*)ddepth.p) == want, "nuts device, no samples kept");
    EXPECT(hipstub_launches_on(stream) == on0 + (want == LR_OK ? 3 : 0), "nuts device: one launch per call, on the caller's stream");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
}

// every kernel family on one model, host buffers and device buffers, with and without statistics
static void run_all_kinds(lr_model* m, const Data& d, int64_t C, int dtype, void* stream, int precision, int mode = LR_MODE_AUTO, int group = 0) {
    const size_t es = dtype == LR_F32 ? 4 : 8;
    std::vector<unsigned char> state((size_t)C * d.p * es, 0), out((size_t)2 * C * d.p * es);
    std::vector<double> lp(C, -INFINITY), vec(d.p, 1.0);
    std::vector<uint32_t> acc(C, 0);
    lr_run_opts o{};
    o.n_chains = C; o.thin = 2; o.iters = 2; o.seed = 7; o.mode = mode; o.group = group; o.precision = precision; o.stream = nullptr;
    EXPECT(lr_run_hmc(m, state.data(), 0.01, 3, vec.data(), &o, out.data(), acc.data()) == LR_OK, "hmc host C=%lld", (long long)C);
    EXPECT(lr_run_mala(m, state.data(), lp.data(), 1e-3, vec.data(), &o, out.data(), acc.data()) == LR_OK, "mala host");
    EXPECT(lr_run_rwmh(m, state.data(), lp.data(), vec.data(), &o, out.data(), acc.data()) == LR_OK, "rwmh host");
    EXPECT(lr_run_ul(m, state.data(), 1e-3, vec.data(), &o, nullptr, acc.data()) == LR_OK, "ul host, no samples kept");
    // on-device buffers on the caller's stream, with a statistics window
    Dev dstate((size_t)C * d.p * es), dlp((size_t)C * 8), dout((size_t)2 * C * d.p * es), dacc((size_t)C * 4), dstats((size_t)2 * C * 2 * d.p * 8);
    EXPECT(dstate.p && dlp.p && dout.p && dacc.p && dstats.p, "device buffers");
    o.on_device = 1; o.stream = stream; o.stats = (double*)dstats.p; o.stats_batch = 1; o.stats_first = 0; o.stats_slots = 2;
    EXPECT(lr_run_hmc(m, dstate.p, 0.01, 4, vec.data(), &o, dout.p, (uint32_t*)dacc.p) == LR_OK, "hmc device + stats");
    o.iter_offset = 4; o.stats_first = 0;
    EXPECT(lr_run_mala(m, dstate.p, (double*)dlp.p, 1e-3, vec.data(), &o, nullptr, (uint32_t*)dacc.p) == LR_OK, "mala device, stats only");
    std::vector<double> piv(d.p, 0.0), sums((size_t)LR_STATS_ROWS * d.p);
    EXPECT(lr_stats_reduce(0, (double*)dstats.p, C, d.p, 1, 2, piv.data(), sums.data(), stream) == LR_OK, "stats reduce");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    // closures
    std::vector<unsigned char> beta((size_t)C * d.p * es, 0), ll((size_t)C * es), grad((size_t)C * d.p * es);
    lr_run_opts e{};
    e.n_chains = C; e.mode = LR_MODE_AUTO;
    EXPECT(lr_eval(m, beta.data(), ll.data(), ll.data(), ll.data(), grad.data(), &e) == LR_OK, "eval");
    EXPECT(lr_eval(m, beta.data(), nullptr, nullptr, ll.data(), nullptr, &e) == LR_OK, "eval lpost only");
    run_nuts(m, d, C, dtype, stream, mode, group);
}

static void scenario_models() {
    struct Shape { int64_t n; int p; int64_t C; const char* what; };
    const Shape shapes[] = {
        {200, 8, 64, "Pima-sized: rows in registers"}, {200, 8, 4096, "one wave per SIMD"}, {200, 8, 5120, "a two-part plan (head + remainder on a side stream)"},
        {200, 8, 20480, "matrix-core head + remainder"}, {1500, 8, 4096, "rows in LDS / matrix-core operands in LDS"}, {3000, 8, 2048, "operand images in device memory"},
        {20000, 8, 256, "tall: stepwise engine + matrix-pipe interior image"}, {300, 24, 600, "17 <= p <= 32"}, {1000, 12, 4096, "9 <= p <= 16 matrix-core"},
        {600, 64, 300, "wide p = 64: row-split / trajectory kernels"}, {700, 128, 1100, "wide p = 128, several chain blocks"}, {37, 3, 5, "tiny"}, {1, 1, 1, "n = p = C = 1"}};
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (const Shape& s : shapes) {
        const Data d = make_data(s.n, s.p, (unsigned)(s.n + s.p));
        for (int dtype : {LR_F32, LR_F64}) {
            lr_model* m = nullptr;
            EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), dtype, 0, &m) == LR_OK, "create %s dtype %d", s.what, dtype);
            if (!m) continue;
            int64_t n; int32_t p, dt, dev, pp, fmt;
            EXPECT(lr_model_info(m, &n, &p, &dt, &dev, &pp) == LR_OK && n == d.n && p == d.p && dt == dtype && pp >= p, "info");
            EXPECT(lr_model_interior_format(m, &fmt) == LR_OK, "interior format");
            char buf[64];
            EXPECT(lr_model_debug_opts(m, buf, sizeof buf) == LR_OK, "debug opts");
            for (int prec : {LR_PREC_AUTO, LR_PREC_FULL}) run_all_kinds(m, d, s.C, dtype, stream, prec);
            // the plan as the caller sees it, for a run and for a shard of it
            lr_run_opts o{};
            o.n_chains = s.C; o.thin = 1; o.iters = 1; o.mode = LR_MODE_AUTO;
            lr_plan_info pi{};
            EXPECT(lr_plan_run_info(m, LR_KIND_HMC, &o, &pi) == LR_OK, "plan info");
            if (s.C >= 4) {  // a shard planned as the whole run is (plan_chains / plan_first), straddling a two-part split if there is one
                lr_run_opts sh = o;
                sh.n_chains = s.C / 2; sh.chain_offset = 1000 + s.C / 4; sh.plan_chains = (int32_t)s.C; sh.plan_first = 1000; sh.thin = 2; sh.iters = 1; sh.seed = 3;
                const size_t es = dtype == LR_F32 ? 4 : 8;
                std::vector<unsigned char> st((size_t)sh.n_chains * d.p * es, 0), out((size_t)sh.n_chains * d.p * es);
                std::vector<double> vec(d.p, 1.0);
                std::vector<uint32_t> acc(sh.n_chains, 0);
                EXPECT(lr_run_hmc(m, st.data(), 0.01, 2, vec.data(), &sh, out.data(), acc.data()) == LR_OK, "planned shard of %s", s.what);
            }
            if (d.p <= 32 && d.n >= 8) {
                std::vector<double> b(d.p, 0.0), g(d.p), h((size_t)d.p * d.p);
                double lpost = 0;
                EXPECT(lr_hessian(m, b.data(), &lpost, g.data(), h.data(), stream) == LR_OK, "hessian");
            }
            lr_model_destroy(m);
        }
    }
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
}

// forced engines: every (mode, group) the planner accepts on a small model, both dtypes
static void scenario_forced_variants() {
    const Data d = make_data(200, 8, 5);
    for (int dtype : {LR_F32, LR_F64}) {
        lr_model* m = nullptr;
        EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), dtype, 0, &m) == LR_OK, "create");
        int ok = 0;
        for (int mode : {LR_MODE_REG, LR_MODE_LDS, LR_MODE_GLOBAL, LR_MODE_MFMA, LR_MODE_STEPWISE, LR_MODE_MIXED})
            for (int g : {0, 1, 2, 4, 8, 16, 32, 64}) {
                int32_t mo, go, ro;
                if (lr_plan(m, 300, g, mode, &mo, &go, &ro) != LR_OK) continue;  // (an LR_ERR_* with a message: not a finding)
                ++ok;
                run_all_kinds(m, d, 300, dtype, nullptr, LR_PREC_AUTO, mode, g);
            }
        EXPECT(ok >= 8, "forced variants accepted: %d", ok);
        lr_model_destroy(m);
    }
}

// two chain sets of ONE model on two streams, interleaved launches (per-stream workspaces and side slots), then a second model
static void scenario_two_streams() {
    const Data d = make_data(200, 8, 11), w = make_data(600, 64, 12);
    lr_model *m = nullptr, *mw = nullptr;
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_OK, "create");
    EXPECT(lr_model_create(w.X.data(), w.y.data(), w.n, w.p, w.sd.data(), LR_F32, 0, &mw) == LR_OK, "create wide");
    void *s1 = nullptr, *s2 = nullptr;
    EXPECT(lr_stream_create(0, &s1) == LR_OK && lr_stream_create(0, &s2) == LR_OK, "streams");
    const int64_t C = 5120;  // (a two-part plan: each launch forks to a side stream and joins)
    Dev st1((size_t)C * 8 * 4), st2((size_t)C * 8 * 4), acc((size_t)C * 4), wst((size_t)300 * 64 * 4), wacc(300 * 4);
    std::vector<double> vec(8, 1.0), wvec(64, 1.0);
    lr_run_opts o{};
    o.n_chains = C; o.thin = 1; o.iters = 1; o.seed = 1; o.on_device = 1; o.mode = LR_MODE_AUTO; o.precision = LR_PREC_FULL;
    lr_run_opts ow = o;
    ow.n_chains = 300; ow.precision = LR_PREC_AUTO;
    const long before1 = hipstub_launches_on(s1), before2 = hipstub_launches_on(s2);
    for (int it = 0; it < 4; ++it) {
        o.iter_offset = it;
        o.stream = s1;
        EXPECT(lr_run_hmc(m, st1.p, 0.01, 3, vec.data(), &o, nullptr, (uint32_t*)acc.p) == LR_OK, "set 1");
        o.stream = s2;
        EXPECT(lr_run_hmc(m, st2.p, 0.01, 3, vec.data(), &o, nullptr, (uint32_t*)acc.p) == LR_OK, "set 2");
        ow.stream = it & 1 ? s1 : s2;  // the stepwise engine's workspaces are per stream as well
        ow.iter_offset = it;
        EXPECT(lr_run_hmc(mw, wst.p, 0.01, 4, wvec.data(), &ow, nullptr, (uint32_t*)wacc.p) == LR_OK, "wide on alternating streams");
    }
    EXPECT(hipstub_launches_on(s1) > before1 && hipstub_launches_on(s2) > before2, "launches went to the callers' streams");
    EXPECT(lr_stream_sync(0, s1) == LR_OK && lr_stream_sync(0, s2) == LR_OK, "sync");
    lr_model_destroy(mw);
    lr_model_destroy(m);
    EXPECT(lr_stream_destroy(0, s1) == LR_OK && lr_stream_destroy(0, s2) == LR_OK, "destroy streams");
}

static void scenario_errors() {
    const Data d = make_data(50, 4, 3);
    lr_model* m = nullptr;
    std::vector<double> bad = d.y;
    bad[3] = 0.5;
    EXPECT(lr_model_create(nullptr, d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_ERR_INVALID, "NULL X");
    EXPECT(lr_model_create(d.X.data(), bad.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_ERR_INVALID, "y not 0/1");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), 0, d.p, d.sd.data(), LR_F32, 0, &m) == LR_ERR_INVALID, "n = 0");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, 1000, d.sd.data(), LR_F32, 0, &m) == LR_ERR_UNSUPPORTED, "p too large");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), 7, 0, &m) == LR_ERR_INVALID, "dtype");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 5, &m) == LR_ERR_HIP, "device ordinal");
    std::vector<double> sd0 = d.sd;
    sd0[1] = 0.0;
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, sd0.data(), LR_F32, 0, &m) == LR_ERR_INVALID, "prior sd 0");
    std::vector<double> Xn = d.X;
    Xn[7] = NAN;
    EXPECT(lr_model_create(Xn.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_ERR_INVALID, "NaN in X");
    EXPECT(m == nullptr, "no model came out of a failed create");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_OK, "create");
    std::vector<float> st(64 * 4, 0.f), out(64 * 4);
    std::vector<double> lp(64, 0.0), vec(4, 1.0), neg(4, -1.0);
    std::vector<uint32_t> acc(64, 0);
    lr_run_opts o{};
    o.n_chains = 64; o.thin = 1; o.iters = 1; o.mode = LR_MODE_AUTO;
    EXPECT(lr_run_hmc(nullptr, st.data(), 0.1, 2, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "NULL model");
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), nullptr, out.data(), acc.data()) == LR_ERR_INVALID, "NULL opts");
    EXPECT(lr_run_hmc(m, nullptr, 0.1, 2, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "NULL state");
    EXPECT(lr_run_hmc(m, st.data(), -0.1, 2, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "eps < 0");
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 0, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "l = 0");
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, neg.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "dmm < 0");
    EXPECT(lr_run_mala(m, st.data(), nullptr, 1e-3, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "mala without lp_state");
    EXPECT(lr_run_mala(m, st.data(), lp.data(), 0.0, vec.data(), &o, out.data(), acc.data()) == LR_ERR_INVALID, "dt = 0");
    EXPECT(lr_run_rwmh(m, st.data(), lp.data(), nullptr, &o, out.data(), acc.data()) == LR_ERR_INVALID, "NULL prop_sd");
    lr_run_opts b = o;
    b.n_chains = 0;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "0 chains");
    b = o; b.thin = 0;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "thin = 0");
    b = o; b.precision = 9;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "precision");
    b = o; b.group = 3;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "group 3");
    b = o; b.mode = LR_MODE_MFMA;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_UNSUPPORTED, "no matrix-core kernel at p = 4");
    b = o; b.chain_offset = (int64_t)1 << 33;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "chain id beyond 32 bits");
    // the containment rule of a planned shard: [chain_offset, chain_offset + n) inside [plan_first, plan_first + plan_chains)
    b = o; b.plan_chains = 100; b.plan_first = 50; b.chain_offset = 40;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "shard starts before the planned run");
    b.chain_offset = 100;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "shard ends beyond the planned run");
    b.chain_offset = 60; b.n_chains = 40;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_OK, "a shard inside the planned run");
    b = o; b.plan_chains = -1;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "plan_chains < 0");
    std::vector<double> stats(2 * 64 * 2 * 4);
    b = o; b.stats = stats.data(); b.stats_batch = 0; b.stats_slots = 2;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "stats_batch = 0");
    b.stats_batch = 1; b.stats_first = 2; b.iters = 1;
    EXPECT(lr_run_hmc(m, st.data(), 0.1, 2, vec.data(), &b, out.data(), acc.data()) == LR_ERR_INVALID, "statistics window overrun");
    // lr_run_nuts: its own parameters first, then the options and arrays as every run, then what its one kernel family cannot do
    std::vector<lr_nuts_counters> cnt(64, lr_nuts_counters{});
    std::vector<int8_t> dep(64);
    EXPECT(lr_run_nuts(nullptr, st.data(), 0.1, 3, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts NULL model");
    EXPECT(lr_run_nuts(m, st.data(), 0.0, 3, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts eps = 0");
    EXPECT(lr_run_nuts(m, st.data(), NAN, 3, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts eps NaN");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 0, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts max_depth = 0");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, LR_NUTS_MAX_DEPTH + 1, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts max_depth beyond the limit");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, nullptr, &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts NULL dmm");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, neg.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts dmm < 0");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), nullptr, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts NULL opts");
    EXPECT(lr_run_nuts(m, nullptr, 0.1, 3, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts NULL state");
    b = o; b.thin = 0;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts thin = 0");
    b = o; b.group = 3;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts group 3");
    b = o; b.stats = stats.data(); b.stats_batch = 1; b.stats_first = 2; b.stats_slots = 2;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_INVALID, "nuts statistics window overrun");
    b = o; b.group = 8;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_UNSUPPORTED, "nuts on 8 lanes per chain");
    b = o; b.mode = LR_MODE_STEPWISE;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_UNSUPPORTED, "nuts on the stepwise engine");
    b = o; b.mode = LR_MODE_REG;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_UNSUPPORTED, "nuts with rows in registers");
    b = o; b.iters = 0; b.mode = LR_MODE_REG;
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &b, out.data(), cnt.data(), dep.data()) == LR_ERR_UNSUPPORTED, "nuts: refused before 'nothing to do'");
    EXPECT(lr_run_nuts(m, st.data(), 0.1, 3, vec.data(), &o, out.data(), cnt.data(), dep.data()) == LR_OK, "nuts, after all the refusals");
    lr_run_opts e{};
    e.n_chains = 64;
    EXPECT(lr_eval(m, nullptr, out.data(), nullptr, nullptr, nullptr, &e) == LR_ERR_INVALID, "eval NULL beta");
    int32_t a, g2, r;
    EXPECT(lr_plan(m, 0, 0, LR_MODE_AUTO, &a, &g2, &r) == LR_ERR_INVALID, "plan for 0 chains");
    EXPECT(lr_plan_run(m, 9, &o, &a, &g2, &r) == LR_ERR_INVALID, "plan for an unknown kind");
    EXPECT(lr_stats_reduce(0, nullptr, 64, 4, 1, 1, vec.data(), vec.data(), nullptr) == LR_ERR_INVALID, "stats reduce NULL");
    float ms;
    void* ev = nullptr;
    EXPECT(lr_event_create(0, &ev) == LR_OK, "event");
    const long bw = hipstub_bad_waits();
    EXPECT(lr_event_elapsed_ms(0, ev, ev, &ms) != LR_OK, "elapsed time of an event never recorded");
    g_deliberate_bad_waits += hipstub_bad_waits() - bw;
    EXPECT(lr_event_record(0, ev, nullptr) == LR_OK && lr_event_elapsed_ms(0, ev, ev, &ms) == LR_OK, "record + elapsed");
    EXPECT(lr_event_destroy(0, ev) == LR_OK, "event destroy");
    EXPECT(std::strlen(lr_last_error()) > 0, "the last failure left a message");
    lr_model_destroy(m);
    lr_model_destroy(nullptr);  // (as free(NULL))
    hipstub_set_devices(0);
    EXPECT(lr_device_count() == 0, "no device");
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_ERR_HIP, "create without a device");
    hipstub_set_devices(1);
}

// the k-th device allocation of lr_model_create fails, for every k the creation makes: LR_ERR_NOMEM, nothing leaked, no handle returned
static void scenario_failing_allocations() {
    struct Shape { int64_t n; int p; int dtype; };
    for (const Shape& s : {Shape{200, 8, LR_F32}, Shape{3000, 8, LR_F32}, Shape{20000, 8, LR_F32}, Shape{700, 128, LR_F32}, Shape{700, 128, LR_F64}, Shape{300, 24, LR_F64}}) {
        const Data d = make_data(s.n, s.p, 99);
        lr_model* m = nullptr;
        const long m0 = hipstub_mallocs();
        EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), s.dtype, 0, &m) == LR_OK, "create");
        const long made = hipstub_mallocs() - m0;
        lr_model_destroy(m);
        const long live0 = hipstub_live_allocs();
        for (long k = 1; k <= made; ++k) {
            m = nullptr;
            int rc;
            { FailMallocAt failing(k); rc = lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), s.dtype, 0, &m); }
            EXPECT(rc == LR_ERR_NOMEM && m == nullptr, "allocation %ld of %ld fails (n=%lld p=%d): rc %d", k, made, (long long)s.n, s.p, rc);
            EXPECT(hipstub_live_allocs() == live0, "allocation %ld of %ld fails: %ld device buffers leaked", k, made, hipstub_live_allocs() - live0);
            if (m) lr_model_destroy(m);
        }
        // ... and a failing allocation inside a run (sample buffer, statistics, workspaces): an error, then the model still works
        EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), s.dtype, 0, &m) == LR_OK, "create again");
        const size_t es = s.dtype == LR_F32 ? 4 : 8;
        const int64_t C = 128;
        std::vector<unsigned char> st((size_t)C * d.p * es, 0), out((size_t)C * d.p * es);
        std::vector<double> vec(d.p, 1.0);
        std::vector<uint32_t> acc(C, 0);
        lr_run_opts o{};
        o.n_chains = C; o.thin = 1; o.iters = 1; o.mode = LR_MODE_AUTO;
        const long r0 = hipstub_mallocs();
        EXPECT(lr_run_hmc(m, st.data(), 0.01, 2, vec.data(), &o, out.data(), acc.data()) == LR_OK, "run");
        const long in_run = hipstub_mallocs() - r0;
        lr_model_destroy(m);
        for (long k = 1; k <= in_run; ++k) {
            EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), s.dtype, 0, &m) == LR_OK, "fresh model");
            const long before = hipstub_live_allocs();
            int rc;
            { FailMallocAt failing(k); rc = lr_run_hmc(m, st.data(), 0.01, 2, vec.data(), &o, out.data(), acc.data()); }
            EXPECT(rc == LR_ERR_NOMEM || rc == LR_ERR_HIP, "allocation %ld of %ld inside the run fails: rc %d", k, in_run, rc);
            EXPECT(lr_run_hmc(m, st.data(), 0.01, 2, vec.data(), &o, out.data(), acc.data()) == LR_OK, "the model runs after a failed run");
            lr_model_destroy(m);
            EXPECT(hipstub_live_allocs() <= before - 1, "a failed run leaked past the model's destruction");
        }
    }
}

// The host-pointer path of a run, of lr_run_nuts and of lr_eval stages one device buffer per array the caller gave and none for one left
// out.  The k-th of them fails, for every k: LR_ERR_NOMEM, nothing leaked, and the same call works next time.
static void scenario_failing_staged_allocations() {
    const Data d = make_data(200, 8, 98);
    const int64_t C = 96;
    for (int dtype : {LR_F32, LR_F64}) {
        lr_model* m = nullptr;
        EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), dtype, 0, &m) == LR_OK, "create");
        if (!m) continue;
        const size_t es = dtype == LR_F32 ? 4 : 8;
        std::vector<unsigned char> st((size_t)C * d.p * es, 0), out((size_t)2 * C * d.p * es), ll((size_t)3 * C * es), grad((size_t)C * d.p * es);
        std::vector<double> lp(C, -INFINITY), vec(d.p, 1.0), stats((size_t)2 * C * 2 * d.p, 0.0);
        std::vector<uint32_t> acc(C, 0);
        std::vector<lr_nuts_counters> cnt(C, lr_nuts_counters{});
        std::vector<int8_t> dep((size_t)2 * C);
        lr_run_opts o{};
        o.n_chains = C; o.thin = 1; o.iters = 2; o.mode = LR_MODE_AUTO;
        lr_run_opts os = o;
        os.stats = stats.data(); os.stats_batch = 1; os.stats_slots = 2;
        struct Call { const char* what; long arrays; std::function<int()> run; };
        const Call calls[] = {
            {"mala, every array + statistics", 5, [&] { return lr_run_mala(m, st.data(), lp.data(), 1e-3, vec.data(), &os, out.data(), acc.data()); }},
            {"hmc, the state alone", 1, [&] { return lr_run_hmc(m, st.data(), 0.01, 2, vec.data(), &o, nullptr, nullptr); }},
            {"nuts, every array + statistics", 5, [&] { return lr_run_nuts(m, st.data(), 0.01, 3, vec.data(), &os, out.data(), cnt.data(), dep.data()); }},
            {"nuts, the state and the depths", 2, [&] { return lr_run_nuts(m, st.data(), 0.01, 3, vec.data(), &o, nullptr, nullptr, dep.data()); }},
            {"eval, every output", 5, [&] { return lr_eval(m, st.data(), ll.data(), ll.data() + C * es, ll.data() + 2 * C * es, grad.data(), &o); }},
            {"eval, lpost alone", 2, [&] { return lr_eval(m, st.data(), nullptr, nullptr, ll.data(), nullptr, &o); }}};
        for (const Call& c : calls) {
            const long live0 = hipstub_live_allocs(), m0 = hipstub_mallocs();
            EXPECT(c.run() == LR_OK, "%s", c.what);
            const long made = hipstub_mallocs() - m0;
            EXPECT(made == c.arrays && hipstub_live_allocs() == live0, "%s: %ld device buffers staged for %ld arrays, %ld left behind", c.what, made, c.arrays, hipstub_live_allocs() - live0);
            for (long k = 1; k <= made; ++k) {
                int rc;
                { FailMallocAt failing(k); rc = c.run(); }
                EXPECT(rc == LR_ERR_NOMEM, "%s: allocation %ld of %ld fails: rc %d", c.what, k, made, rc);
                EXPECT(hipstub_live_allocs() == live0, "%s: allocation %ld of %ld fails: %ld device buffers leaked", c.what, k, made, hipstub_live_allocs() - live0);
                EXPECT(c.run() == LR_OK, "%s: the call works after a failed one", c.what);
            }
        }
        lr_model_destroy(m);
    }
}

// A rank of a multi-GPU job works on device LOCAL_RANK, not 0 (bench.py, logreg_amd.distributed): everything the library allocates,
// creates and launches for a model on device 1 must happen with device 1 current -- a path that forgot its hipSetDevice would put a
// workspace or a launch on device 0 and only an 8-GPU node would ever show it.
static void scenario_second_device() {
    hipstub_set_devices(2);
    EXPECT(lr_device_count() == 2 && lr_device_cus(1) == 256, "two devices");
    char info[256];
    EXPECT(lr_device_info(1, info, sizeof info) == LR_OK && std::strstr(info, "pci=") != nullptr, "device info of device 1");
    void* stream = nullptr;
    const long zero0 = hipstub_work_on_device(0);
    EXPECT(lr_stream_create(1, &stream) == LR_OK, "stream on device 1");
    struct Shape { int64_t n; int p; int64_t C; };
    for (const Shape& s : {Shape{200, 8, 5120}, Shape{20000, 8, 256}, Shape{600, 64, 300}, Shape{300, 24, 600}}) {
        const Data d = make_data(s.n, s.p, 77);
        for (int dtype : {LR_F32, LR_F64}) {
            lr_model* m = nullptr;
            EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), dtype, 1, &m) == LR_OK, "create on device 1");
            if (!m) continue;
            int64_t n; int32_t p, dt, dev, pp;
            EXPECT(lr_model_info(m, &n, &p, &dt, &dev, &pp) == LR_OK && dev == 1, "the model reports device 1");
            const size_t es = dtype == LR_F32 ? 4 : 8;
            void *st = nullptr, *lp = nullptr, *out = nullptr, *acc = nullptr, *stats = nullptr;
            EXPECT(lr_malloc(1, (size_t)s.C * d.p * es, &st) == LR_OK && lr_malloc(1, (size_t)s.C * 8, &lp) == LR_OK && lr_malloc(1, (size_t)s.C * d.p * es, &out) == LR_OK &&
                   lr_malloc(1, (size_t)s.C * 4, &acc) == LR_OK && lr_malloc(1, (size_t)s.C * 2 * d.p * 8, &stats) == LR_OK, "buffers on device 1");
            std::vector<double> vec(d.p, 1.0);
            lr_run_opts o{};
            o.n_chains = s.C; o.thin = 1; o.iters = 1; o.on_device = 1; o.stream = stream; o.mode = LR_MODE_AUTO;
            o.stats = (double*)stats; o.stats_batch = 1; o.stats_slots = 1;
            for (int prec : {LR_PREC_AUTO, LR_PREC_FULL}) {
                o.precision = prec;
                EXPECT(lr_run_hmc(m, st, 0.01, 3, vec.data(), &o, out, (uint32_t*)acc) == LR_OK, "hmc on device 1");
                EXPECT(lr_run_mala(m, st, (double*)lp, 1e-3, vec.data(), &o, out, (uint32_t*)acc) == LR_OK, "mala on device 1");
            }
            std::vector<double> piv(d.p, 0.0), sums((size_t)LR_STATS_ROWS * d.p);
            EXPECT(lr_stats_reduce(1, (double*)stats, s.C, d.p, 1, 1, piv.data(), sums.data(), stream) == LR_OK, "stats reduce on device 1");
            std::vector<unsigned char> host((size_t)s.C * d.p * es);
            EXPECT(lr_memcpy_d2h(1, host.data(), out, host.size(), stream) == LR_OK && lr_memset(1, acc, 0, (size_t)s.C * 4, stream) == LR_OK, "copies on device 1");
            // (host-pointer convenience path: the library stages through its own device buffers)
            std::vector<unsigned char> hs((size_t)64 * d.p * es, 0), ho((size_t)64 * d.p * es);
            std::vector<uint32_t> ha(64, 0);
            lr_run_opts h{};
            h.n_chains = 64; h.thin = 1; h.iters = 1; h.mode = LR_MODE_AUTO;
            EXPECT(lr_run_hmc(m, hs.data(), 0.01, 2, vec.data(), &h, ho.data(), ha.data()) == LR_OK, "host buffers, model on device 1");
            if (d.p <= 32) {
                std::vector<double> b(d.p, 0.0), g(d.p), hh((size_t)d.p * d.p);
                double lpost;
                EXPECT(lr_hessian(m, b.data(), &lpost, g.data(), hh.data(), stream) == LR_OK, "hessian on device 1");
            }
            EXPECT(lr_stream_sync(1, stream) == LR_OK, "sync");
            for (void* q : {st, lp, out, acc, stats}) EXPECT(lr_free(1, q) == LR_OK, "free");
            lr_model_destroy(m);
        }
    }
    EXPECT(lr_stream_destroy(1, stream) == LR_OK, "stream destroy");
    EXPECT(hipstub_work_on_device(0) == zero0, "%ld allocations / creations / launches happened with device 0 current while working on device 1",
           hipstub_work_on_device(0) - zero0);
    EXPECT(hipstub_work_on_device(1) > 200, "work counted on device 1: %ld", hipstub_work_on_device(1));
    hipstub_set_devices(1);
}

// ---- the accumulators of kept draws -------------------------------------------------------------------------------------------------
// One accumulator behind closures, so that one life cycle and one failing-allocation sweep serve all four.  feed takes `items` draws (of a
// model) or time steps (of a block) from a zero-filled buffer; result makes every result call the accumulator has and reports the draws held
// and the first cell of the table.
struct Acc {
    std::string name;
    size_t item_bytes;          // one draw / one time step as the caller hands it over
    const char* kernel;         // the kernel every staged piece launches once (marginals: once per 4096 steps of it)
    std::function<int()> create;
    std::function<bool()> made;
    std::function<int(const void*, int64_t, int, void*)> feed;
    std::function<int(int64_t*, double*)> result;
    std::function<int()> reset;
    std::function<void()> destroy;
};

static Acc acc_predict(lr_model* const* m, int p, int dtype, int64_t rows, bool own_rows) {
    auto h = std::make_shared<lr_predict*>(nullptr);
    auto X = std::make_shared<std::vector<double>>((size_t)rows * p, 0.25);
    auto y = std::make_shared<std::vector<double>>((size_t)rows, 1.0);
    Acc a;
    a.name = own_rows ? "predict, the model's own rows" : "predict, new rows";
    a.item_bytes = (size_t)p * (dtype == LR_F32 ? 4 : 8);
    a.kernel = "k_predict_partial";
    a.create = [=] { return lr_predict_create(*m, own_rows ? nullptr : X->data(), own_rows ? nullptr : y->data(), rows, h.get()); };
    a.made = [=] { return *h != nullptr; };
    a.feed = [=](const void* src, int64_t S, int on_device, void* st) { return lr_predict_accumulate(*h, src, S, on_device, st); };
    a.result = [=](int64_t* n, double* first) {
        std::vector<double> t((size_t)LR_PRED_ROWS * rows, 7.0);
        const int rc = lr_predict_result(*h, t.data(), n);
        *first = t[0];
        return rc;
    };
    a.reset = [=] { return lr_predict_reset(*h); };
    a.destroy = [=] { lr_predict_destroy(*h); *h = nullptr; };
    return a;
}
static Acc acc_loo(lr_model* const* m, int p, int dtype, int64_t rows, int64_t max_draws) {
    auto h = std::make_shared<lr_loo*>(nullptr);
    Acc a;
    a.name = "loo";
    a.item_bytes = (size_t)p * (dtype == LR_F32 ? 4 : 8);
    a.kernel = "k_loo_fill";
    a.create = [=] { return lr_loo_create(*m, max_draws, h.get()); };
    a.made = [=] { return *h != nullptr; };
    a.feed = [=](const void* src, int64_t S, int on_device, void* st) { return lr_loo_accumulate(*h, src, S, on_device, st); };
    a.result = [=](int64_t* n, double* first) {
        std::vector<double> t((size_t)LR_LOO_ROWS * rows, 7.0);
        int64_t held = -1;
        int rc = lr_loo_loglik(*h, nullptr, &held);  // (the count alone)
        std::vector<unsigned char> ll((size_t)(held > 0 ? held : 0) * rows * 8 + 1);
        if (!rc) rc = lr_loo_loglik(*h, ll.data(), nullptr);
        if (!rc) rc = lr_loo_result(*h, t.data(), n);
        else *n = held;
        *first = t[0];
        return rc;
    };
    a.reset = [=] { return lr_loo_reset(*h); };
    a.destroy = [=] { lr_loo_destroy(*h); *h = nullptr; };
    return a;
}
static Acc acc_acf(int dtype, int64_t C, int p, int max_lag) {
    auto h = std::make_shared<lr_acf*>(nullptr);
    Acc a;
    a.name = "acf";
    a.item_bytes = (size_t)C * p * (dtype == LR_F32 ? 4 : 8);
    a.kernel = "k_acf_accumulate";
    a.create = [=] { return lr_acf_create(0, dtype, C, p, max_lag, h.get()); };
    a.made = [=] { return *h != nullptr; };
    a.feed = [=](const void* src, int64_t k, int on_device, void* st) { return lr_acf_accumulate(*h, src, k, on_device, st); };
    a.result = [=](int64_t* n, double* first) {
        std::vector<double> sums((size_t)LR_ACF_ROWS(max_lag) * p, 7.0), ess((size_t)C * p, 7.0);
        int rc = lr_acf_result(*h, sums.data(), nullptr, n);
        if (!rc) rc = lr_acf_result(*h, sums.data(), ess.data(), n);
        *first = sums[0];
        return rc;
    };
    a.reset = [=] { return lr_acf_reset(*h); };
    a.destroy = [=] { lr_acf_destroy(*h); *h = nullptr; };
    return a;
}
static Acc acc_marg(int dtype, int64_t C, int p, int bins) {
    auto h = std::make_shared<lr_marg*>(nullptr);
    auto lo = std::make_shared<std::vector<double>>((size_t)p, -1.0);
    auto hi = std::make_shared<std::vector<double>>((size_t)p, 1.0);
    Acc a;
    a.name = "marginals";
    a.item_bytes = (size_t)C * p * (dtype == LR_F32 ? 4 : 8);
    a.kernel = "k_marg_accumulate";
    a.create = [=] { return lr_marg_create(0, dtype, C, p, bins, lo->data(), hi->data(), h.get()); };
    a.made = [=] { return *h != nullptr; };
    a.feed = [=](const void* src, int64_t k, int on_device, void* st) { return lr_marg_accumulate(*h, src, k, on_device, st); };
    a.result = [=](int64_t* n, double* first) {
        std::vector<uint64_t> counts((size_t)p * LR_MARG_COLS(bins), 7);
        std::vector<double> t((size_t)LR_MARG_ROWS * p, 7.0);
        int rc = lr_marg_result(*h, counts.data(), nullptr, n);
        if (!rc) rc = lr_marg_result(*h, nullptr, t.data(), n);
        if (!rc) rc = lr_marg_result(*h, counts.data(), t.data(), n);
        *first = t[0];
        return rc;
    };
    a.reset = [=] { return lr_marg_reset(*h); };
    a.destroy = [=] { lr_marg_destroy(*h); *h = nullptr; };
    return a;
}

// create, host and device input on a stream, the result before the first draw and after, reset, more draws, destroy
static void accumulator_life(const Acc& a, const void* zeros, void* stream) {
    int64_t n = -1;
    double first = 0;
    EXPECT(a.create() == LR_OK && a.made(), "%s: create", a.name.c_str());
    if (!a.made()) return;
    EXPECT(a.result(&n, &first) == LR_OK && n == 0 && std::isnan(first), "%s: NaN before the first draw (n %lld, %g)", a.name.c_str(), (long long)n, first);
    Dev dev(7 * a.item_bytes);
    EXPECT(dev.p != nullptr, "device input");
    const long l0 = hipstub_launches_on(stream), k0 = hipstub_launches_of(a.kernel);
    EXPECT(a.feed(zeros, 5, 0, stream) == LR_OK, "%s: host input", a.name.c_str());
    EXPECT(a.feed(dev.p, 7, 1, stream) == LR_OK, "%s: device input", a.name.c_str());
    EXPECT(hipstub_launches_of(a.kernel) == k0 + 2 && hipstub_launches_on(stream) >= l0 + 2, "%s: one piece each, on the caller's stream", a.name.c_str());
    EXPECT(a.result(&n, &first) == LR_OK && n == 12, "%s: result of 12 (n %lld)", a.name.c_str(), (long long)n);
    EXPECT(a.reset() == LR_OK && a.result(&n, &first) == LR_OK && n == 0 && std::isnan(first), "%s: reset", a.name.c_str());
    EXPECT(a.feed(zeros, 3, 0, nullptr) == LR_OK && a.result(&n, &first) == LR_OK && n == 3, "%s: more draws after a reset, on the NULL stream", a.name.c_str());
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    a.destroy();
}

// host input one item longer than one staging piece of `piece` items: two pieces in one call, as the same items in two calls cut there
static void accumulator_two_pieces(const Acc& a, int64_t piece, const void* zeros, void* stream) {
    int64_t n = -1;
    double first = 0;
    EXPECT(a.create() == LR_OK && a.made(), "%s: create", a.name.c_str());
    if (!a.made()) return;
    const long k0 = hipstub_launches_of(a.kernel);
    EXPECT(a.feed(zeros, piece, 0, stream) == LR_OK && hipstub_launches_of(a.kernel) == k0 + 1, "%s: %lld items are one piece", a.name.c_str(), (long long)piece);
    EXPECT(a.feed(zeros, 1, 0, stream) == LR_OK && hipstub_launches_of(a.kernel) == k0 + 2, "%s: one more", a.name.c_str());
    EXPECT(a.reset() == LR_OK, "reset");
    EXPECT(a.feed(zeros, piece + 1, 0, stream) == LR_OK && hipstub_launches_of(a.kernel) == k0 + 4, "%s: %lld items are two pieces", a.name.c_str(), (long long)piece + 1);
    EXPECT(a.result(&n, &first) == LR_OK && n == piece + 1, "%s: all of them counted (n %lld)", a.name.c_str(), (long long)n);
    a.destroy();
}

// the k-th device allocation fails, for every k that create, accumulate (first use and regrow) and result make: LR_ERR_NOMEM, the draw
// count as it was, nothing leaked, the accumulator usable afterwards
static void accumulator_failing_allocations(const Acc& a, const void* zeros) {
    int64_t n = -1;
    double first = 0;
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(a.create() == LR_OK && a.made(), "%s: create", a.name.c_str());
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(a.feed(zeros, 3, 0, nullptr) == LR_OK, "%s: feed", a.name.c_str());
    const long in_feed = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(a.feed(zeros, 40, 0, nullptr) == LR_OK, "%s: a longer feed", a.name.c_str());
    const long in_regrow = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(a.result(&n, &first) == LR_OK && n == 43, "%s: result", a.name.c_str());
    const long in_result = hipstub_mallocs() - m0;
    a.destroy();
    EXPECT(hipstub_live_allocs() == live0, "%s: %ld device buffers outlive the accumulator", a.name.c_str(), hipstub_live_allocs() - live0);
    EXPECT(in_create >= 1 && in_feed >= 1 && in_regrow >= 1 && in_regrow <= in_feed, "%s: allocations %ld / %ld / %ld / %ld", a.name.c_str(), in_create, in_feed, in_regrow, in_result);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = a.create(); }
        EXPECT(rc == LR_ERR_NOMEM && !a.made(), "%s: allocation %ld of %ld of create fails: rc %d", a.name.c_str(), k, in_create, rc);
        if (a.made()) a.destroy();
        EXPECT(hipstub_live_allocs() == live0, "%s: allocation %ld of create fails: %ld device buffers leaked", a.name.c_str(), k, hipstub_live_allocs() - live0);
    }
    for (int regrow = 0; regrow < 2; ++regrow)
        for (long k = 1; k <= (regrow ? in_regrow : in_feed); ++k) {  // (a workspace that is large enough does not grow again)
            EXPECT(a.create() == LR_OK && a.made(), "%s: fresh", a.name.c_str());
            if (regrow) EXPECT(a.feed(zeros, 3, 0, nullptr) == LR_OK, "%s: feed", a.name.c_str());
            const int64_t before = regrow ? 3 : 0;
            int rc;
            { FailMallocAt failing(k); rc = a.feed(zeros, 40, 0, nullptr); }
            EXPECT(rc == LR_ERR_NOMEM, "%s: allocation %ld of accumulate fails (regrow %d): rc %d", a.name.c_str(), k, regrow, rc);
            EXPECT(a.result(&n, &first) == LR_OK && n == before, "%s: the count stays %lld after a failed accumulate (n %lld)", a.name.c_str(), (long long)before, (long long)n);
            EXPECT(a.feed(zeros, 40, 0, nullptr) == LR_OK && a.result(&n, &first) == LR_OK && n == before + 40, "%s: usable after a failed accumulate", a.name.c_str());
            a.destroy();
            EXPECT(hipstub_live_allocs() == live0, "%s: a failed accumulate leaked %ld device buffers", a.name.c_str(), hipstub_live_allocs() - live0);
        }
    for (long k = 1; k <= in_result; ++k) {
        EXPECT(a.create() == LR_OK && a.made() && a.feed(zeros, 43, 0, nullptr) == LR_OK, "%s: fresh", a.name.c_str());
        int rc;
        { FailMallocAt failing(k); rc = a.result(&n, &first); }
        EXPECT(rc == LR_ERR_NOMEM && n == 43, "%s: allocation %ld of %ld of result fails: rc %d, n %lld", a.name.c_str(), k, in_result, rc, (long long)n);
        EXPECT(a.result(&n, &first) == LR_OK && n == 43 && a.feed(zeros, 2, 0, nullptr) == LR_OK, "%s: usable after a failed result", a.name.c_str());
        a.destroy();
        EXPECT(hipstub_live_allocs() == live0, "%s: a failed result leaked %ld device buffers", a.name.c_str(), hipstub_live_allocs() - live0);
    }
}

static void scenario_accumulators() {
    // zero-filled input for everything below: 65 time steps of the 8192 x 64 float64 block (64 steps of it are one 256 MB staging piece)
    const int64_t bigC = 8192;
    const int bigp = 64;
    const std::vector<unsigned char> zeros((size_t)65 * bigC * bigp * 8, 0);
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (int dtype : {LR_F32, LR_F64}) {
        for (int p : {8, 5}) {  // p == P, and draws padded to the kernel width
            const Data d = make_data(16, p, 31);
            lr_model* m = nullptr;
            EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), dtype, 0, &m) == LR_OK, "create");
            for (const Acc& a : {acc_predict(&m, p, dtype, d.n, true), acc_predict(&m, p, dtype, 9, false), acc_loo(&m, p, dtype, d.n, 100)}) {
                accumulator_life(a, zeros.data(), stream);
                accumulator_failing_allocations(a, zeros.data());
            }
            // the accumulators own their buffers: destroyed after the model
            const Acc pr = acc_predict(&m, p, dtype, 9, false), lo = acc_loo(&m, p, dtype, d.n, 10);
            EXPECT(pr.create() == LR_OK && lo.create() == LR_OK && pr.feed(zeros.data(), 4, 0, stream) == LR_OK && lo.feed(zeros.data(), 4, 0, stream) == LR_OK, "feed");
            lr_model_destroy(m);
            pr.destroy();
            lo.destroy();
        }
        for (const Acc& a : {acc_acf(dtype, 37, 5, 3), acc_marg(dtype, 37, 5, 8)}) {
            accumulator_life(a, zeros.data(), stream);
            accumulator_failing_allocations(a, zeros.data());
        }
        // the PSIS stage alone, host and device matrix
        std::vector<double> table((size_t)LR_LOO_ROWS * 6);
        Dev dll((size_t)30 * 6 * 8);
        EXPECT(lr_psis(0, zeros.data(), 30, 6, dtype, 0, table.data(), stream) == LR_OK && lr_psis(0, dll.p, 30, 6, dtype, 1, table.data(), stream) == LR_OK, "psis");
        EXPECT(lr_psis(0, zeros.data(), 5000, 3, dtype, 0, table.data(), nullptr) == LR_OK, "psis, the kernel of long tails");
        for (long k = 1; k <= 3; ++k) {
            const long live0 = hipstub_live_allocs();
            int rc;
            { FailMallocAt failing(k); rc = lr_psis(0, zeros.data(), 30, 6, dtype, 0, table.data(), stream); }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_live_allocs() == live0, "psis: allocation %ld fails: rc %d, %ld leaked", k, rc, hipstub_live_allocs() - live0);
        }
    }
    // input one item longer than one staging piece.  Blocks: 256 MB / (8192 x 64 x 8 bytes) = 64 steps.  Draws of a float64 model with p = 100
    // (kernel width 128): 256 MB / (128 x 8 bytes) = 262144 draws
    accumulator_two_pieces(acc_acf(LR_F64, bigC, bigp, 1), 64, zeros.data(), stream);
    accumulator_two_pieces(acc_marg(LR_F64, bigC, bigp, 8), 64, zeros.data(), stream);
    {
        const Data d = make_data(16, 100, 32);
        lr_model* m = nullptr;
        EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F64, 0, &m) == LR_OK, "create");
        accumulator_two_pieces(acc_predict(&m, 100, LR_F64, d.n, true), 262144, zeros.data(), stream);
        accumulator_two_pieces(acc_loo(&m, 100, LR_F64, d.n, 2 * 262145), 262144, zeros.data(), stream);
        lr_model_destroy(m);
    }
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
}

// every refused argument of the accumulators, through its error return
static void scenario_accumulator_errors() {
    const Data d = make_data(16, 5, 33);
    lr_model* m = nullptr;
    EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), LR_F32, 0, &m) == LR_OK, "create");
    std::vector<double> X((size_t)4 * d.p, 0.5), y(4, 1.0), t(4096, 0.0), lo(5, -1.0), hi(5, 1.0);
    std::vector<float> draws((size_t)64 * d.p, 0.f);
    int64_t n = 0;

    lr_predict* pp = nullptr;
    EXPECT(lr_predict_create(nullptr, X.data(), y.data(), 4, &pp) == LR_ERR_INVALID && lr_predict_create(m, X.data(), y.data(), 4, nullptr) == LR_ERR_INVALID, "predict: NULL model / out");
    EXPECT(lr_predict_create(m, X.data(), y.data(), 0, &pp) == LR_ERR_INVALID, "predict: r = 0");
    EXPECT(lr_predict_create(m, X.data(), y.data(), (int64_t)1 << 60, &pp) == LR_ERR_UNSUPPORTED, "predict: r beyond the grid");
    EXPECT(lr_predict_create(m, nullptr, y.data(), d.n, &pp) == LR_ERR_INVALID, "predict: labels without rows");
    EXPECT(lr_predict_create(m, nullptr, nullptr, d.n + 1, &pp) == LR_ERR_INVALID, "predict: the model's own rows, another count");
    y[2] = 0.5;
    EXPECT(lr_predict_create(m, X.data(), y.data(), 4, &pp) == LR_ERR_INVALID, "predict: a label that is not 0 / 1");
    y[2] = 0.0;
    X[7] = INFINITY;
    EXPECT(lr_predict_create(m, X.data(), y.data(), 4, &pp) == LR_ERR_INVALID && lr_predict_create(m, X.data(), nullptr, 4, &pp) == LR_ERR_INVALID, "predict: a row that is not finite");
    X[7] = 0.5;
    EXPECT(pp == nullptr, "no accumulator came out of a failed create");
    EXPECT(lr_predict_create(m, X.data(), nullptr, 4, &pp) == LR_OK, "predict: rows without labels");
    EXPECT(lr_predict_accumulate(nullptr, draws.data(), 4, 0, nullptr) == LR_ERR_INVALID && lr_predict_accumulate(pp, nullptr, 4, 0, nullptr) == LR_ERR_INVALID, "predict: NULL accumulator / draws");
    EXPECT(lr_predict_accumulate(pp, draws.data(), 0, 0, nullptr) == LR_ERR_INVALID && lr_predict_accumulate(pp, draws.data(), -2, 0, nullptr) == LR_ERR_INVALID, "predict: S <= 0");
    EXPECT(lr_predict_result(nullptr, t.data(), &n) == LR_ERR_INVALID && lr_predict_result(pp, nullptr, &n) == LR_ERR_INVALID && lr_predict_reset(nullptr) == LR_ERR_INVALID, "predict: NULL result / reset");
    EXPECT(lr_predict_accumulate(pp, draws.data(), 6, 0, nullptr) == LR_OK && lr_predict_result(pp, t.data(), nullptr) == LR_OK && std::isnan(t[2 * 4]) && !std::isnan(t[4]),
           "predict: without labels the rows of the labels stay NaN");
    lr_predict_destroy(pp);
    lr_predict_destroy(nullptr);

    lr_loo* lp = nullptr;
    EXPECT(lr_loo_create(nullptr, 10, &lp) == LR_ERR_INVALID && lr_loo_create(m, 10, nullptr) == LR_ERR_INVALID, "loo: NULL model / out");
    EXPECT(lr_loo_create(m, 0, &lp) == LR_ERR_INVALID && lr_loo_create(m, (int64_t)LR_LOO_MAX_DRAWS + 1, &lp) == LR_ERR_UNSUPPORTED && lp == nullptr, "loo: max_draws");
    EXPECT(lr_loo_create(m, 10, &lp) == LR_OK, "loo: create");
    EXPECT(lr_loo_accumulate(nullptr, draws.data(), 4, 0, nullptr) == LR_ERR_INVALID && lr_loo_accumulate(lp, nullptr, 4, 0, nullptr) == LR_ERR_INVALID, "loo: NULL accumulator / draws");
    EXPECT(lr_loo_accumulate(lp, draws.data(), 0, 0, nullptr) == LR_ERR_INVALID, "loo: S = 0");
    EXPECT(lr_loo_accumulate(lp, draws.data(), 11, 0, nullptr) == LR_ERR_INVALID, "loo: more than max_draws at once");
    EXPECT(lr_loo_accumulate(lp, draws.data(), 6, 0, nullptr) == LR_OK && lr_loo_accumulate(lp, draws.data(), 5, 0, nullptr) == LR_ERR_INVALID, "loo: more than max_draws in all");
    EXPECT(lr_loo_loglik(lp, nullptr, &n) == LR_OK && n == 6, "loo: a refused accumulate leaves the count (n %lld)", (long long)n);
    EXPECT(lr_loo_loglik(nullptr, nullptr, &n) == LR_ERR_INVALID && lr_loo_result(nullptr, t.data(), &n) == LR_ERR_INVALID && lr_loo_result(lp, nullptr, &n) == LR_ERR_INVALID &&
               lr_loo_reset(nullptr) == LR_ERR_INVALID, "loo: NULL loglik / result / reset");
    lr_loo_destroy(lp);
    lr_loo_destroy(nullptr);

    lr_acf* ac = nullptr;
    EXPECT(lr_acf_create(0, LR_F32, 8, 5, 3, nullptr) == LR_ERR_INVALID, "acf: NULL out");
    EXPECT(lr_acf_create(0, LR_F32, 0, 5, 3, &ac) == LR_ERR_INVALID && lr_acf_create(0, LR_F32, 8, 0, 3, &ac) == LR_ERR_INVALID, "acf: C, p");
    for (int lag : {0, 2, LR_ACF_MAX_LAG + 2}) EXPECT(lr_acf_create(0, LR_F32, 8, 5, lag, &ac) == LR_ERR_INVALID, "acf: max_lag %d", lag);
    EXPECT(lr_acf_create(0, 7, 8, 5, 3, &ac) == LR_ERR_INVALID, "acf: dtype");
    EXPECT(lr_acf_create(0, LR_F32, (int64_t)1 << 50, 5, 3, &ac) == LR_ERR_UNSUPPORTED, "acf: series beyond the grid");
    EXPECT(lr_acf_create(5, LR_F32, 8, 5, 3, &ac) == LR_ERR_HIP && lr_acf_create(-1, LR_F32, 8, 5, 3, &ac) == LR_ERR_HIP && ac == nullptr, "acf: device ordinal");
    EXPECT(lr_acf_create(0, LR_F32, 8, 5, 3, &ac) == LR_OK, "acf: create");
    EXPECT(lr_acf_accumulate(nullptr, draws.data(), 2, 0, nullptr) == LR_ERR_INVALID && lr_acf_accumulate(ac, nullptr, 2, 0, nullptr) == LR_ERR_INVALID &&
               lr_acf_accumulate(ac, draws.data(), 0, 0, nullptr) == LR_ERR_INVALID, "acf: NULL accumulator / block, k = 0");
    EXPECT(lr_acf_result(nullptr, t.data(), nullptr, &n) == LR_ERR_INVALID && lr_acf_result(ac, nullptr, nullptr, &n) == LR_ERR_INVALID && lr_acf_reset(nullptr) == LR_ERR_INVALID,
           "acf: NULL result / reset");
    lr_acf_destroy(ac);
    lr_acf_destroy(nullptr);
    ac = nullptr;

    lr_marg* mg = nullptr;
    EXPECT(lr_marg_create(0, LR_F32, 8, 5, 16, lo.data(), hi.data(), nullptr) == LR_ERR_INVALID && lr_marg_create(0, LR_F32, 8, 5, 16, nullptr, hi.data(), &mg) == LR_ERR_INVALID &&
               lr_marg_create(0, LR_F32, 8, 5, 16, lo.data(), nullptr, &mg) == LR_ERR_INVALID, "marginals: NULL out / lo / hi");
    EXPECT(lr_marg_create(0, LR_F32, 0, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_INVALID && lr_marg_create(0, LR_F32, 8, -1, 16, lo.data(), hi.data(), &mg) == LR_ERR_INVALID, "marginals: C, p");
    for (int bins : {0, LR_MARG_MAX_BINS + 1}) EXPECT(lr_marg_create(0, LR_F32, 8, 5, bins, lo.data(), hi.data(), &mg) == LR_ERR_INVALID, "marginals: bins %d", bins);
    EXPECT(lr_marg_create(0, 7, 8, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_INVALID, "marginals: dtype");
    for (double bad : {1.0, 2.0, (double)NAN, (double)INFINITY}) {
        lo[3] = bad;
        EXPECT(lr_marg_create(0, LR_F32, 8, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_INVALID, "marginals: lo = %g, hi = 1", bad);
    }
    lo[3] = -1.0;
    EXPECT(lr_marg_create(0, LR_F32, (int64_t)1 << 50, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_UNSUPPORTED, "marginals: series beyond the grid");
    EXPECT(lr_marg_create(5, LR_F32, 8, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_HIP && mg == nullptr, "marginals: device ordinal");
    EXPECT(lr_marg_create(0, LR_F32, 8, 5, 16, lo.data(), hi.data(), &mg) == LR_OK, "marginals: create");
    EXPECT(lr_marg_accumulate(nullptr, draws.data(), 2, 0, nullptr) == LR_ERR_INVALID && lr_marg_accumulate(mg, nullptr, 2, 0, nullptr) == LR_ERR_INVALID &&
               lr_marg_accumulate(mg, draws.data(), -1, 0, nullptr) == LR_ERR_INVALID, "marginals: NULL accumulator / block, k < 0");
    EXPECT(lr_marg_result(nullptr, nullptr, t.data(), &n) == LR_ERR_INVALID && lr_marg_reset(nullptr) == LR_ERR_INVALID, "marginals: NULL result / reset");
    EXPECT(lr_marg_result(mg, nullptr, nullptr, &n) == LR_OK && n == 0, "marginals: the count alone");
    lr_marg_destroy(mg);
    lr_marg_destroy(nullptr);
    mg = nullptr;

    EXPECT(lr_psis(0, nullptr, 30, 4, LR_F32, 0, t.data(), nullptr) == LR_ERR_INVALID && lr_psis(0, draws.data(), 30, 4, LR_F32, 0, nullptr, nullptr) == LR_ERR_INVALID, "psis: NULL loglik / table");
    EXPECT(lr_psis(0, draws.data(), 0, 4, LR_F32, 0, t.data(), nullptr) == LR_ERR_INVALID && lr_psis(0, draws.data(), 30, 0, LR_F32, 0, t.data(), nullptr) == LR_ERR_INVALID, "psis: S, r");
    EXPECT(lr_psis(0, draws.data(), 30, 4, 7, 0, t.data(), nullptr) == LR_ERR_INVALID, "psis: dtype");
    EXPECT(lr_psis(0, draws.data(), (int64_t)LR_LOO_MAX_DRAWS + 1, 4, LR_F32, 0, t.data(), nullptr) == LR_ERR_UNSUPPORTED, "psis: S beyond LR_LOO_MAX_DRAWS");
    EXPECT(lr_psis(0, draws.data(), 30, 65535ll * 32 + 1, LR_F32, 0, t.data(), nullptr) == LR_ERR_UNSUPPORTED, "psis: r beyond the grid");
    EXPECT(lr_psis(5, draws.data(), 30, 4, LR_F32, 0, t.data(), nullptr) == LR_ERR_HIP, "psis: device ordinal");
    lr_model_destroy(m);
    // without a device: the block accumulators report the failing count, lr_psis that none is visible
    hipstub_set_devices(0);
    EXPECT(lr_acf_create(0, LR_F32, 8, 5, 3, &ac) == LR_ERR_HIP && std::strstr(lr_last_error(), "hipGetDeviceCount") != nullptr, "acf without a device: %s", lr_last_error());
    EXPECT(lr_marg_create(0, LR_F32, 8, 5, 16, lo.data(), hi.data(), &mg) == LR_ERR_HIP && std::strstr(lr_last_error(), "hipGetDeviceCount") != nullptr, "marginals without a device");
    EXPECT(lr_psis(0, draws.data(), 30, 4, LR_F32, 0, t.data(), nullptr) == LR_ERR_HIP && std::strstr(lr_last_error(), "(0 visible)") != nullptr, "psis without a device: %s", lr_last_error());
    EXPECT(ac == nullptr && mg == nullptr, "no accumulator without a device");
    hipstub_set_devices(1);
}

// ---- mode `trace`: which kernels the stepwise engine launches, with which grid, in which order -------------------------------------
// A line per model ("== dtype n p chains [debug option]") and under it one per case, "<case>: <launches>": a launch is the index of its record (kernel name, grid, block, LDS, stream ordinal)
// in the table printed at the end, and a run of repeats is folded, innermost first: "(3 4)*7" is seven times launch 3 then launch 4.
static std::string fold(const std::vector<int>& s, size_t lo, size_t hi) {
    std::string out;
    for (size_t i = lo; i < hi;) {
        size_t bp = 0, br = 1;  // the period and count of the repeat from i on that covers the most launches (ties: the shortest period)
        for (size_t p = 1; p <= (hi - i) / 2; ++p) {
            size_t r = 1;
            while (i + (r + 1) * p <= hi && std::equal(s.begin() + i, s.begin() + i + p, s.begin() + i + r * p)) ++r;
            if (r > 1 && r * p > br * bp) bp = p, br = r;
        }
        if (!out.empty()) out += ' ';
        if (br > 1) {
            out += (bp > 1 ? "(" + fold(s, i, i + bp) + ")" : fold(s, i, i + bp)) + "*" + std::to_string(br);
            i += bp * br;
        } else {
            out += std::to_string(s[i++]);
        }
    }
    return out;
}
struct Trace {
    std::vector<std::string> names, records;
    std::map<std::string, int> name_ix, record_ix;
    void begin() { hipstub_trace_begin(); }
    void end(const std::string& label, int rc) {
        std::vector<int> seq;
        for (long i = 0, k = hipstub_trace_end(); i < k; ++i) {
            const std::string rec = hipstub_trace_record(i), name = rec.substr(0, rec.find(' '));
            if (name_ix.emplace(name, (int)names.size()).second) names.push_back(name);
            const std::string key = std::to_string(name_ix[name]) + rec.substr(rec.find(' '));
            if (record_ix.emplace(key, (int)records.size()).second) records.push_back(key);
            seq.push_back(record_ix[key]);
        }
        if (rc != LR_OK) std::printf("%s: status %d\n", label.c_str(), rc);
        else std::printf("%s: %s\n", label.c_str(), fold(seq, 0, seq.size()).c_str());
    }
    void tables() const {
        for (size_t i = 0; i < records.size(); ++i) std::printf("launch %zu = kernel %s\n", i, records[i].c_str());
        for (size_t i = 0; i < names.size(); ++i) std::printf("kernel %zu = %s\n", i, names[i].c_str());
    }
};
static void mode_trace() {
    struct Shape { int64_t n; int p; int64_t C; int dtype; bool small; };
    const Shape shapes[] = {// the shapes of the planner's trajectory rule and of the tall 16-wave rule (tests/test_planner_cpu.py)
                            {2000, 128, 1024, LR_F32, false}, {3000, 128, 1024, LR_F32, false}, {4096, 128, 1024, LR_F32, false}, {4096, 128, 2048, LR_F32, false},
                            {4096, 128, 3072, LR_F32, false}, {4096, 128, 4096, LR_F32, false}, {4096, 128, 8192, LR_F32, false}, {3000, 64, 1024, LR_F32, false},
                            {5000, 64, 1024, LR_F32, false}, {8000, 64, 2048, LR_F32, false}, {100000, 8, 1024, LR_F32, false}, {100000, 8, 4096, LR_F32, false},
                            // small ones: tall in both dtypes, and the shapes of test_short_trajectories_on_the_reduced_precision_interior_kernels
                            {20000, 8, 256, LR_F32, true}, {20000, 8, 256, LR_F64, true}, {900, 128, 70, LR_F32, true}, {900, 128, 70, LR_F64, true}, {2600, 128, 70, LR_F32, true},
                            {3000, 8, 70, LR_F32, true}, {1500, 20, 70, LR_F32, true}};
    const char* const precs[] = {"auto", "full", "bf16"};  // LR_PREC_AUTO, _FULL, _BF16
    Trace tr;
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (const Shape& s : shapes) {
        Data d = make_data(s.n, s.p, (unsigned)(s.n + s.p));
        const size_t es = s.dtype == LR_F32 ? 4 : 8;
        Dev state((size_t)s.C * d.p * es), out((size_t)2 * s.C * d.p * es), acc((size_t)s.C * sizeof(lr_nuts_counters)), lp((size_t)s.C * 8), depth((size_t)2 * s.C), ll((size_t)3 * s.C * es);
        EXPECT(state.p && out.p && acc.p && lp.p && depth.p && ll.p, "device buffers");
        std::vector<double> vec(d.p, 1.0);
        std::vector<std::string> opts = {""};
        if (s.p > 32) for (const char* o : {"wide_traj=0", "wide_traj=1", "wide_traj=2", "wide_f16=0", "rows beyond f16"}) opts.push_back(o);
        else opts.push_back("tall_mx16=0");
        for (const std::string& opt : opts) {
            const bool big = opt == "rows beyond f16";  // (not an option: the same rows times 2^17, which the half-precision image refuses)
            if (big) for (double& x : d.X) x *= 131072.0;
            setenv("LOGREG_DEBUG_OPTS", big ? "" : opt.c_str(), 1);
            lr_model* m = nullptr;
            EXPECT(lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), s.dtype, 0, &m) == LR_OK, "create n=%lld p=%d %s", (long long)s.n, s.p, opt.c_str());
            if (!m) continue;
            std::printf("== %s n=%lld p=%d C=%lld [%s]\n", s.dtype == LR_F32 ? "f32" : "f64", (long long)s.n, s.p, (long long)s.C, opt.c_str());
            lr_run_opts o{};
            o.n_chains = s.C; o.thin = 2; o.iters = 2; o.seed = 7; o.mode = LR_MODE_STEPWISE; o.on_device = 1; o.stream = stream;
            for (int L : {1, 2, 3, 4, 8})
                for (int prec = 0; prec < 3; ++prec) {
                    o.precision = prec;
                    tr.begin();
                    const int rc = lr_run_hmc(m, state.p, 0.01, L, vec.data(), &o, out.p, (uint32_t*)acc.p);
                    tr.end("L=" + std::to_string(L) + " " + precs[prec], rc);
                }
            o.precision = LR_PREC_AUTO;
            if (s.small && opt.empty()) {  // the other families, lr_eval and NUTS; a shard planned as a larger run
                tr.begin();
                int rc = lr_run_rwmh(m, state.p, (double*)lp.p, vec.data(), &o, out.p, (uint32_t*)acc.p);
                tr.end("rwmh", rc);
                tr.begin();
                rc = lr_run_mala(m, state.p, (double*)lp.p, 1e-3, vec.data(), &o, out.p, (uint32_t*)acc.p);
                tr.end("mala", rc);
                tr.begin();
                rc = lr_run_ul(m, state.p, 1e-3, vec.data(), &o, out.p, (uint32_t*)acc.p);
                tr.end("ul", rc);
                tr.begin();
                rc = lr_eval(m, state.p, ll.p, (char*)ll.p + s.C * es, (char*)ll.p + 2 * s.C * es, out.p, &o);
                tr.end("eval", rc);
                tr.begin();
                rc = lr_run_nuts(m, state.p, 0.01, 3, vec.data(), &o, out.p, (lr_nuts_counters*)acc.p, (int8_t*)depth.p);
                tr.end("nuts depth 3", rc);
            }
            if (opt.empty()) {
                lr_run_opts sh = o;
                sh.n_chains = s.C / 2; sh.chain_offset = s.C / 4; sh.plan_chains = (int32_t)(8 * s.C); sh.plan_first = 0;
                tr.begin();
                const int rc = lr_run_hmc(m, state.p, 0.01, 4, vec.data(), &sh, out.p, (uint32_t*)acc.p);
                tr.end("L=4 auto, half the chains of a run planned for 8 x as many", rc);
            }
            lr_model_destroy(m);
        }
    }
    unsetenv("LOGREG_DEBUG_OPTS");
    EXPECT(lr_stream_sync(0, stream) == LR_OK && lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    tr.tables();
}

static void thread_body(int id, int* fails) {
    const Data d = id == 0 ? make_data(200, 8, 21) : make_data(600, 64, 22);
    lr_model* m = nullptr;
    void* stream = nullptr;
    int bad = 0;
    bad += lr_model_create(d.X.data(), d.y.data(), d.n, d.p, d.sd.data(), id == 0 ? LR_F32 : LR_F64, 0, &m) != LR_OK;
    bad += lr_stream_create(0, &stream) != LR_OK;
    const int64_t C = id == 0 ? 5120 : 300;
    const size_t es = id == 0 ? 4 : 8;
    Dev st((size_t)C * d.p * es), acc((size_t)C * 4), out((size_t)C * d.p * es);
    std::vector<double> vec(d.p, 1.0);
    lr_run_opts o{};
    o.n_chains = C; o.thin = 1; o.iters = 1; o.on_device = 1; o.stream = stream; o.mode = LR_MODE_AUTO; o.precision = id == 0 ? LR_PREC_FULL : LR_PREC_AUTO;
    for (int it = 0; it < 20 && m; ++it) {
        o.iter_offset = it;
        bad += lr_run_hmc(m, st.p, 0.01, 3, vec.data(), &o, out.p, (uint32_t*)acc.p) != LR_OK;
        if (it % 5 == 0) bad += lr_stream_sync(0, stream) != LR_OK;
    }
    lr_model_destroy(m);
    bad += lr_stream_destroy(0, stream) != LR_OK;
    *fails = bad;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "threads") {
        int f0 = 0, f1 = 0;
        std::thread a(thread_body, 0, &f0), b(thread_body, 1, &f1);
        a.join();
        b.join();
        EXPECT(f0 == 0 && f1 == 0, "thread failures %d %d", f0, f1);
    } else if (what == "trace") {
        mode_trace();
    } else {
        scenario_models();
        scenario_forced_variants();
        scenario_two_streams();
        scenario_errors();
        scenario_failing_allocations();
        scenario_failing_staged_allocations();
        scenario_second_device();
        scenario_accumulators();
        scenario_accumulator_errors();
    }
    EXPECT(hipstub_wrong_device() == 0, "%ld uses of another device's stream / event", hipstub_wrong_device());
    EXPECT(hipstub_bad_waits() == g_deliberate_bad_waits, "%ld waits on events that were never recorded", hipstub_bad_waits() - g_deliberate_bad_waits);
    EXPECT(hipstub_bad_launches() == 0, "%ld launches with an invalid configuration or a dead stream", hipstub_bad_launches());
    EXPECT(hipstub_live_allocs() == 0, "%ld device buffers alive at exit", hipstub_live_allocs());
    EXPECT(hipstub_live_streams() == 0 && hipstub_live_events() == 0, "%ld streams, %ld events alive at exit", hipstub_live_streams(), hipstub_live_events());
    std::printf("engine harness (%s): %ld kernel launches (%ld k_chain*, %ld k_tall*, %ld k_wide*), %ld device allocations, %d failures\n", what.c_str(), hipstub_launches(),
                hipstub_launches_of("k_chain"), hipstub_launches_of("k_tall"), hipstub_launches_of("k_wide"), hipstub_mallocs(), g_fail);
    return g_fail ? 1 : 0;
}
