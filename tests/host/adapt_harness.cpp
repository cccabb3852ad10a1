// adapt_harness.cpp -- TEST INFRASTRUCTURE: the host side of the NUTS warm-up (include/logreg_hip_adapt.h; lr_api.hip) as a program of its
// own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory is the host heap) and compiled with
// -fsanitize=address,undefined by tests/test_adapt_cpu.py.  It drives the C ABI: both dtypes, p = 3, 8, 20, create / run in pieces from
// host and device memory / result / trace / destroy, the launch count (three per iteration, on the caller's stream), the schedule, every
// refused argument, and a failing device allocation at EVERY allocation of create and run: LR_ERR_NOMEM, the iteration count unchanged,
// nothing leaked, the handle usable afterwards.  With no-op kernels the numbers are the start values: what is checked is the host logic
// (offsets of the state block staying inside it, staging, every error path), not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"

static void schedule() {
    int32_t ends[LR_ADAPT_MAX_WINDOWS], n = -1, init = -1;
    EXPECT(lr_adapt_schedule(1000, 0, 0, 0, ends, &n, &init) == LR_OK && n == 5 && init == 75 && ends[0] == 100 && ends[1] == 150 && ends[2] == 250 && ends[3] == 450 && ends[4] == 950,
           "W = 1000: %d windows from %d", n, init);
    EXPECT(lr_adapt_schedule(150, 0, 0, 0, ends, &n, &init) == LR_OK && n == 1 && ends[0] == 100, "W = 150");
    EXPECT(lr_adapt_schedule(60, 0, 0, 0, ends, &n, &init) == LR_OK && n == 1 && init == 9 && ends[0] == 54, "W = 60");
    EXPECT(lr_adapt_schedule(19, 0, 0, 0, ends, &n, nullptr) == LR_OK && n == 0, "W = 19");
    EXPECT(lr_adapt_schedule(2000000000, 1, 1, 1, ends, &n, &init) == LR_OK && n >= 1 && n <= LR_ADAPT_MAX_WINDOWS && ends[n - 1] == 1999999999, "a long warm-up stays inside ends[]");
    EXPECT(lr_adapt_schedule(0, 0, 0, 0, ends, &n, &init) == LR_ERR_INVALID && lr_adapt_schedule(10, -1, 0, 0, ends, &n, &init) == LR_ERR_INVALID &&
               lr_adapt_schedule(10, 0, 0, 0, nullptr, &n, &init) == LR_ERR_INVALID && lr_adapt_schedule(10, 0, 0, 0, ends, nullptr, &init) == LR_ERR_INVALID, "refused");
}

// create / run in pieces / result / trace / destroy
static void life(int dtype, int p, int64_t C, int W, void* stream) {
    lr_model* m = model(dtype, p);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    lr_adapt* h = nullptr;
    lr_adapt_opts ao = adapt_opts(W);
    std::vector<double> dmm0((size_t)p, 2.0);
    ao.dmm0 = dmm0.data();
    ao.eps0 = 0.25;
    EXPECT(lr_adapt_create(m, C, &ao, &h) == LR_OK && h, "create (C %lld, p %d, W %d)", (long long)C, p, W);
    if (h) {
        double eps = -1;
        std::vector<double> dmm((size_t)p, -1.0);
        lr_adapt_info info;
        EXPECT(lr_adapt_result(h, &eps, dmm.data(), &info) == LR_OK && eps == 0.25 && dmm[0] == 2.0 && dmm[p - 1] == 2.0 && info.iterations == 0 && info.windows == 0, "the start values");
        int32_t ends[LR_ADAPT_MAX_WINDOWS], nw = 0;
        EXPECT(lr_adapt_schedule(W, 0, 0, 0, ends, &nw, nullptr) == LR_OK && info.n_windows == nw, "the handle's schedule is lr_adapt_schedule's (%d, %d)", info.n_windows, nw);
        std::vector<unsigned char> state(C * p * es, 0), out((size_t)W * C * p * es, 0);
        std::vector<lr_nuts_counters> cnt((size_t)C);
        std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
        std::vector<int8_t> depth((size_t)W * C, 0);
        std::vector<double> astat((size_t)W * C, 0.0);
        lr_run_opts ho = run_opts(C, 0, nullptr), dopt = run_opts(C, 1, stream);
        const long n0 = hipstub_launches(), s0 = hipstub_launches_on(stream), k0 = hipstub_launches_of("k_nuts"), a0 = hipstub_launches_of("k_adapt_partial"), u0 = hipstub_launches_of("k_adapt_update");
        const int64_t first = W > 8 ? 7 : W - 1;
        EXPECT(lr_adapt_run(h, state.data(), 0, 5, &ho, nullptr, nullptr, nullptr, nullptr) == LR_OK, "nothing to do");
        EXPECT(lr_adapt_run(h, state.data(), 1, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "one iteration, host pointers, every array");
        if (first > 0) EXPECT(lr_adapt_run(h, state.data(), first, 5, &ho, nullptr, nullptr, nullptr, nullptr) == LR_OK, "%lld iterations, host pointers, the state alone", (long long)first);
        Dev dstate(C * p * es), dout((size_t)W * C * p * es), dast((size_t)W * C * 8);
        EXPECT(dstate.p && dout.p && dast.p, "device arrays");
        const int64_t rest = W - 1 - first;
        const long before = hipstub_launches_on(stream);
        if (rest > 0) EXPECT(lr_adapt_run(h, dstate.p, rest, 5, &dopt, dout.p, nullptr, nullptr, static_cast<double*>(dast.p)) == LR_OK, "the rest from device memory");
        EXPECT(hipstub_launches_on(stream) == before + 3 * (rest > 0 ? rest : 0) && hipstub_launches_on(stream) >= s0, "three launches per iteration on the caller's stream");
        EXPECT(hipstub_launches() - n0 == 3L * W && hipstub_launches_of("k_nuts") - k0 == W && hipstub_launches_of("k_adapt_partial") - a0 == W && hipstub_launches_of("k_adapt_update") - u0 == W,
               "%ld launches for %d iterations", hipstub_launches() - n0, W);
        EXPECT(lr_adapt_result(h, &eps, dmm.data(), &info) == LR_OK && info.iterations == W, "all %d iterations counted (%lld)", W, (long long)info.iterations);
        EXPECT(lr_adapt_result(h, nullptr, nullptr, nullptr) == LR_OK, "result with nothing asked");
        auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
        EXPECT(refused(lr_adapt_run(h, state.data(), 1, 5, &ho, nullptr, nullptr, nullptr, nullptr), "remain"), "no iteration is left");
        std::vector<double> trace((size_t)W * LR_ADAPT_TRACE_COLS, 7.0), metric((size_t)(nw ? nw : 1) * 2 * p, 7.0);
        EXPECT(lr_adapt_trace(h, trace.data(), metric.data()) == LR_OK && trace[0] != 7.0 && trace.back() != 7.0 && (nw == 0 || (metric[0] != 7.0 && metric.back() != 7.0)), "trace and metric are written whole");
        EXPECT(lr_adapt_trace(h, nullptr, nullptr) == LR_OK && lr_adapt_trace(h, trace.data(), nullptr) == LR_OK && lr_adapt_trace(h, nullptr, metric.data()) == LR_OK, "each alone");
        EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
        lr_adapt_destroy(h);
    }
    lr_model_destroy(m);
}

static void failing_allocations(int dtype, int p, int64_t C) {
    lr_model* m = model(dtype, p);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int W = 30;
    lr_adapt* h = nullptr;
    lr_adapt_opts ao = adapt_opts(W);
    lr_adapt_info info;
    const long live0 = hipstub_live_allocs();
    std::vector<unsigned char> state(C * p * es, 0), out((size_t)W * C * p * es, 0);
    std::vector<lr_nuts_counters> cnt((size_t)C);
    std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
    std::vector<int8_t> depth((size_t)W * C, 0);
    std::vector<double> astat((size_t)W * C, 0.0);
    lr_run_opts ho = run_opts(C, 0, nullptr);
    long m0 = hipstub_mallocs();
    EXPECT(lr_adapt_create(m, C, &ao, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_adapt_run(h, state.data(), 2, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "run");
    const long in_run = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_adapt_run(h, state.data(), 9, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "a longer run");
    const long in_regrow = hipstub_mallocs() - m0;
    lr_adapt_destroy(h);
    h = nullptr;
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the handle", hipstub_live_allocs() - live0);
    EXPECT(in_create >= 1 && in_run >= 5 && in_regrow >= 3 && in_regrow <= in_run, "allocations %ld / %ld / %ld", in_create, in_run, in_regrow);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = lr_adapt_create(m, C, &ao, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h, "allocation %ld of %ld of create fails: rc %d", k, in_create, rc);
        if (h) lr_adapt_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "allocation %ld of create fails: %ld device buffers leaked", k, hipstub_live_allocs() - live0);
    }
    for (int regrow = 0; regrow < 2; ++regrow)
        for (long k = 1; k <= (regrow ? in_regrow : in_run); ++k) {
            EXPECT(lr_adapt_create(m, C, &ao, &h) == LR_OK && h, "fresh");
            if (regrow) EXPECT(lr_adapt_run(h, state.data(), 2, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "run");
            const int64_t before = regrow ? 2 : 0;
            const long l0 = hipstub_launches();
            int rc;
            { FailMallocAt failing(k); rc = lr_adapt_run(h, state.data(), 9, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()); }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == l0, "allocation %ld of run fails (regrow %d): rc %d, %ld launches", k, regrow, rc, hipstub_launches() - l0);
            EXPECT(lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK && info.iterations == before, "the count stays %lld after a failed run (%lld)", (long long)before, (long long)info.iterations);
            EXPECT(lr_adapt_run(h, state.data(), 9, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK && lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK &&
                       info.iterations == before + 9, "usable after a failed run");
            lr_adapt_destroy(h);
            h = nullptr;
            EXPECT(hipstub_live_allocs() == live0, "a failed run leaked %ld device buffers", hipstub_live_allocs() - live0);
        }
    lr_model_destroy(m);
}

static void errors() {
    lr_model* m = model(LR_F32, 5);
    lr_model* wide = model(LR_F32, 40, 64);
    if (!m || !wide) return;
    lr_adapt* h = nullptr;
    lr_adapt_opts ao = adapt_opts(40);
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    const long mallocs0 = hipstub_mallocs();
    EXPECT(refused(lr_adapt_create(nullptr, 8, &ao, &h), "NULL") && refused(lr_adapt_create(m, 8, nullptr, &h), "NULL") && refused(lr_adapt_create(m, 8, &ao, nullptr), "NULL"), "NULL model / opts / out");
    EXPECT(refused(lr_adapt_create(m, 0, &ao, &h), "positive") && refused(lr_adapt_create(m, -2, &ao, &h), "positive"), "C");
    EXPECT(lr_adapt_create(m, (int64_t)1 << 40, &ao, &h) == LR_ERR_UNSUPPORTED, "chains beyond the grid");
    {
        lr_adapt_opts b = ao;
        b.W = 0;
        EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "W must"), "W");
        for (int which = 0; which < 3; ++which) {
            b = ao;
            (which == 0 ? b.init_buffer : which == 1 ? b.term_buffer : b.base_window) = -1;
            EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "buffers"), "a negative buffer (%d)", which);
        }
        for (double bad : {-0.1, 1.0, 1.5, (double)NAN}) {
            b = ao;
            b.delta = bad;
            EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "delta"), "delta = %g", bad);
        }
        for (double bad : {-1.0, (double)INFINITY, (double)NAN}) {
            b = ao;
            b.eps0 = bad;
            EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "eps0"), "eps0 = %g", bad);
            for (int which = 0; which < 3; ++which) {
                b = ao;
                (which == 0 ? b.gamma : which == 1 ? b.t0 : b.kappa) = bad;
                EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "gamma, t0 and kappa"), "gamma / t0 / kappa (%d) = %g", which, bad);
            }
        }
        std::vector<double> d(5, 1.0);
        for (double bad : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
            d[2] = bad;
            b = ao;
            b.dmm0 = d.data();
            EXPECT(refused(lr_adapt_create(m, 8, &b, &h), "dmm0[2]"), "dmm0 = %g", bad);
        }
    }
    EXPECT(lr_adapt_create(wide, 8, &ao, &h) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "p = 40 > 32") != nullptr, "a wide model");
    EXPECT(h == nullptr && hipstub_mallocs() == mallocs0, "refused before any device access");
    EXPECT(lr_adapt_create(m, 8, &ao, &h) == LR_OK && h, "create");
    std::vector<float> state(8 * 5, 0.f);
    std::vector<double> stats(4096, 0.0);
    lr_run_opts o = run_opts(8, 0, nullptr);
    const long l0 = hipstub_launches();
    EXPECT(refused(lr_adapt_run(nullptr, state.data(), 1, 5, &o, nullptr, nullptr, nullptr, nullptr), "NULL") && refused(lr_adapt_run(h, nullptr, 1, 5, &o, nullptr, nullptr, nullptr, nullptr), "NULL") &&
               refused(lr_adapt_run(h, state.data(), 1, 5, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL"), "NULL handle / state / opts");
    EXPECT(refused(lr_adapt_run(h, state.data(), -1, 5, &o, nullptr, nullptr, nullptr, nullptr), "remain") && refused(lr_adapt_run(h, state.data(), 41, 5, &o, nullptr, nullptr, nullptr, nullptr), "remain"), "iters");
    EXPECT(refused(lr_adapt_run(h, state.data(), 1, 0, &o, nullptr, nullptr, nullptr, nullptr), "max_depth") && refused(lr_adapt_run(h, state.data(), 1, 11, &o, nullptr, nullptr, nullptr, nullptr), "max_depth"), "max_depth");
    {
        lr_run_opts b = o;
        b.n_chains = 7;
        EXPECT(refused(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr), "n_chains"), "another chain count");
        b = o;
        b.stats = stats.data();
        EXPECT(refused(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr), "stats"), "streaming statistics");
        b = o;
        b.chain_offset = -1;
        EXPECT(refused(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr), "offsets"), "a negative chain offset");
        b = o;
        b.mode = 4;  // LR_MODE_STEPWISE
        EXPECT(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "stepwise") != nullptr, "plan_nuts' refusal of a forced mode");
        b = o;
        b.group = 8;
        EXPECT(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "group 8") != nullptr, "plan_nuts' refusal of a forced lane count");
        b = o;  // iters, thin and iter_offset are ignored
        b.iters = -5;
        b.thin = 0;
        b.iter_offset = -3;
        EXPECT(lr_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_OK, "iters / thin / iter_offset of the options are not read");
    }
    lr_adapt_info info;
    EXPECT(hipstub_launches() == l0 + 3 && lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK && info.iterations == 1, "refused calls enqueued nothing");
    EXPECT(refused(lr_adapt_result(nullptr, nullptr, nullptr, &info), "NULL") && refused(lr_adapt_trace(nullptr, nullptr, nullptr), "NULL"), "NULL result / trace");
    lr_adapt_destroy(h);
    lr_adapt_destroy(nullptr);
    {   // rows and checkpoints beyond the LDS: refused by plan_nuts at the first run
        lr_model* tall = model(LR_F64, 20, 1200);
        h = nullptr;
        if (tall) {
            std::vector<double> st(8 * 20, 0.0);
            EXPECT(lr_adapt_create(tall, 8, &ao, &h) == LR_OK && h, "create on a tall model");
            if (h) EXPECT(lr_adapt_run(h, st.data(), 1, 10, &o, nullptr, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "LDS") != nullptr, "rows beyond the LDS");
            lr_adapt_destroy(h);
            lr_model_destroy(tall);
        }
    }
    hipstub_set_devices(0);
    h = nullptr;
    EXPECT(lr_adapt_create(m, 8, &ao, &h) == LR_ERR_HIP && h == nullptr, "without a device");
    hipstub_set_devices(1);
    lr_model_destroy(m);
    lr_model_destroy(wide);
}

int main() {
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    schedule();
    for (int dtype : {LR_F32, LR_F64})
        for (int p : {3, 8, 20}) {
            life(dtype, p, 37, 60, stream);
            life(dtype, p, 1025, 150, stream);
            life(dtype, p, 1, 19, stream);
            life(dtype, p, 300, 1, stream);
            failing_allocations(dtype, p, 300);
        }
    errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("adapt harness", "k_adapt_update");
}
