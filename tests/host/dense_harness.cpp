// dense_harness.cpp -- TEST INFRASTRUCTURE: the host side of NUTS under a dense metric (include/logreg_hip_dense.h; lr_api.hip, lr_dense.h)
// as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory is the host heap)
// and compiled with -fsanitize=address,undefined by tests/test_nuts_dense_cpu.py, after the pattern of adapt_harness.cpp.  It drives the
// C ABI: lr_dense_factor at p = 1 .. 32 and its refusals; lr_run_nuts_dense in both dtypes at p = 3, 8, 20 from host and device memory,
// the factor image kept per stream (one allocation, reused while inv_metric stays, rewritten in place when it changes), every refused
// argument ahead of any device access, a failing allocation at every allocation of a host-pointer call; the warm-up handle created,
// run in pieces across its window ends (two more launches per window iteration), read and destroyed, with a failing allocation at every
// allocation of create.  With no-op kernels what is checked is the host logic (offsets, staging, lifetimes, error paths), not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"
#include "logreg_hip_dense.h"

// a well-conditioned symmetric positive definite matrix: a tridiagonal correlation scaled by unequal standard deviations
static std::vector<double> spd(int p, double off = 0.4) {
    std::vector<double> s((size_t)p * p, 0.0);
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            const double r = i == j ? 1.0 : i - j == 1 ? off : 0.0;
            s[(size_t)i * p + j] = s[(size_t)j * p + i] = r * (0.5 + 0.25 * i) * (0.5 + 0.25 * j);
        }
    return s;
}

static void factor() {
    for (int p : {1, 2, 3, 8, 17, 32}) {
        const std::vector<double> sig = spd(p);
        std::vector<double> s((size_t)p), R((size_t)p * p), A((size_t)p * p);
        EXPECT(lr_dense_factor(p, sig.data(), s.data(), R.data(), A.data()) == LR_OK, "factor p = %d", p);
        // (A / s) (A / s)^T Sigma = I
        double worst = 0;
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) {
                double acc = 0;  // (B B^T Sigma)_ij, B = A / s
                for (int k = 0; k < p; ++k) {
                    double bbt = 0;
                    for (int c = 0; c < p; ++c) bbt += A[(size_t)i * p + c] / s[i] * A[(size_t)k * p + c] / s[k];
                    acc += bbt * sig[(size_t)k * p + j];
                }
                worst = std::fmax(worst, std::fabs(acc - (i == j ? 1.0 : 0.0)));
            }
        EXPECT(worst < 1e-12, "p = %d: (A / s)(A / s)^T Sigma differs from I by %g", p, worst);
        EXPECT(lr_dense_factor(p, sig.data(), nullptr, nullptr, nullptr) == LR_OK, "nothing asked (p = %d)", p);
        if (p > 1) {  // only the lower triangle is read
            std::vector<double> up = sig;
            up[1] = NAN;
            EXPECT(lr_dense_factor(p, up.data(), s.data(), nullptr, nullptr) == LR_OK, "a NaN above the diagonal is not read");
        }
    }
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    std::vector<double> s2 = spd(3);
    EXPECT(refused(lr_dense_factor(3, nullptr, nullptr, nullptr, nullptr), "NULL"), "NULL");
    EXPECT(refused(lr_dense_factor(0, s2.data(), nullptr, nullptr, nullptr), "1..32") && refused(lr_dense_factor(33, s2.data(), nullptr, nullptr, nullptr), "1..32"), "p");
    s2[3] = NAN;
    EXPECT(refused(lr_dense_factor(3, s2.data(), nullptr, nullptr, nullptr), "not finite"), "NaN");
    s2 = spd(3);
    s2[8] = INFINITY;
    EXPECT(refused(lr_dense_factor(3, s2.data(), nullptr, nullptr, nullptr), "not finite"), "inf");
    s2 = spd(3);
    s2[4] = 0.0;
    EXPECT(refused(lr_dense_factor(3, s2.data(), nullptr, nullptr, nullptr), "> 0"), "a zero diagonal");
    const double indef[4] = {1.0, 2.0, 2.0, 1.0}, singular[4] = {4.0, 4.0, 4.0, 4.0};
    EXPECT(refused(lr_dense_factor(2, indef, nullptr, nullptr, nullptr), "positive definite"), "indefinite");
    EXPECT(refused(lr_dense_factor(2, singular, nullptr, nullptr, nullptr), "positive definite"), "rank-deficient");
}

static void runs(int dtype, int p, int64_t C, void* stream) {
    lr_model* m = model(dtype, p);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int D = 5;
    const std::vector<double> sig = spd(p), sig2 = spd(p, 0.3);
    std::vector<unsigned char> state(C * p * es, 0), out((size_t)2 * C * p * es, 0);
    std::vector<lr_nuts_counters> cnt((size_t)C);
    std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
    std::vector<int8_t> depth((size_t)2 * C, 0);
    std::vector<double> stats((size_t)4 * C * 2 * p, 0.0);
    lr_run_opts o = run_opts(C, 0, nullptr, 2);
    const long k0 = hipstub_launches_of("k_nuts_dense"), d0 = hipstub_launches_of("k_nuts<");
    long m0 = hipstub_mallocs();
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig.data(), &o, out.data(), cnt.data(), depth.data()) == LR_OK, "host, every array");
    const long first = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig.data(), &o, out.data(), cnt.data(), depth.data()) == LR_OK, "host, again");
    EXPECT(hipstub_mallocs() - m0 == first - 1, "the factor image is kept: %ld then %ld allocations", first, hipstub_mallocs() - m0);
    m0 = hipstub_mallocs();
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig2.data(), &o, out.data(), cnt.data(), depth.data()) == LR_OK, "host, another metric");
    EXPECT(hipstub_mallocs() - m0 == first - 1, "... and rewritten in place");
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig.data(), &o, nullptr, nullptr, nullptr) == LR_OK, "host, the state alone");
    lr_run_opts os = o;
    os.stats = stats.data();
    os.stats_batch = 2;
    os.stats_slots = 4;
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig.data(), &os, nullptr, cnt.data(), nullptr) == LR_OK, "host, statistics and counters");
    lr_run_opts oz = run_opts(C, 0, nullptr, 0);
    EXPECT(lr_run_nuts_dense(m, state.data(), 0.01, D, sig.data(), &oz, out.data(), cnt.data(), depth.data()) == LR_OK, "no iterations");
    Dev dstate(C * p * es), dout((size_t)2 * C * p * es), dcnt(C * sizeof(lr_nuts_counters)), ddepth((size_t)2 * C);
    EXPECT(dstate.p && dout.p && dcnt.p && ddepth.p, "device arrays");
    lr_run_opts od = run_opts(C, 1, stream, 2);
    const long s0 = hipstub_launches_on(stream);
    m0 = hipstub_mallocs();
    EXPECT(lr_run_nuts_dense(m, dstate.p, 0.01, D, sig.data(), &od, dout.p, (lr_nuts_counters*)dcnt.p, (int8_t*)ddepth.p) == LR_OK, "device, every array");
    EXPECT(lr_run_nuts_dense(m, dstate.p, 0.01, D, sig.data(), &od, nullptr, nullptr, nullptr) == LR_OK, "device, the state alone");
    EXPECT(hipstub_mallocs() - m0 == 1 && hipstub_launches_on(stream) == s0 + 2, "device pointers: one factor image for the stream, one launch per call (%ld allocations, %ld launches)",
           hipstub_mallocs() - m0, hipstub_launches_on(stream) - s0);
    EXPECT(hipstub_launches_of("k_nuts_dense") - k0 == 7 && hipstub_launches_of("k_nuts<") == d0, "the dense kernel ran 7 times, the diagonal one never (%ld, %ld)",
           hipstub_launches_of("k_nuts_dense") - k0, hipstub_launches_of("k_nuts<") - d0);
    // a failing allocation at each one of a host-pointer call on a fresh model (its factor image among them)
    lr_model* fresh = model(dtype, p);
    if (fresh) {
        const long live0 = hipstub_live_allocs();
        for (long k = 1; k <= first; ++k) {
            const long l0 = hipstub_launches();
            int rc;
            { FailMallocAt failing(k); rc = lr_run_nuts_dense(fresh, state.data(), 0.01, D, sig.data(), &os, out.data(), cnt.data(), depth.data()); }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == l0, "allocation %ld of %ld fails: rc %d", k, first, rc);
            EXPECT(hipstub_live_allocs() <= live0 + 1, "allocation %ld fails: %ld buffers beyond the model's factor image", k, hipstub_live_allocs() - live0);
        }
        EXPECT(lr_run_nuts_dense(fresh, state.data(), 0.01, D, sig.data(), &os, out.data(), cnt.data(), depth.data()) == LR_OK, "usable afterwards");
        lr_model_destroy(fresh);
    }
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    lr_model_destroy(m);
}

static void run_errors() {
    lr_model* m = model(LR_F32, 5);
    lr_model* wide = model(LR_F32, 40, 64);
    if (!m || !wide) return;
    const std::vector<double> sig = spd(5);
    std::vector<float> st(8 * 5, 0.f), out(2 * 8 * 5, 0.f);
    std::vector<lr_nuts_counters> cnt(8);
    std::vector<int8_t> dep(16);
    lr_run_opts o = run_opts(8, 0, nullptr, 2);
    const long mallocs0 = hipstub_mallocs(), l0 = hipstub_launches();
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    EXPECT(refused(lr_run_nuts_dense(nullptr, st.data(), 0.1, 3, sig.data(), &o, nullptr, nullptr, nullptr), "NULL"), "NULL model");
    EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.0, 3, sig.data(), &o, nullptr, nullptr, nullptr), "eps") && refused(lr_run_nuts_dense(m, st.data(), NAN, 3, sig.data(), &o, nullptr, nullptr, nullptr), "eps"), "eps");
    EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 0, sig.data(), &o, nullptr, nullptr, nullptr), "max_depth") &&
               refused(lr_run_nuts_dense(m, st.data(), 0.1, LR_NUTS_MAX_DEPTH + 1, sig.data(), &o, nullptr, nullptr, nullptr), "max_depth"), "max_depth");
    EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 3, nullptr, &o, nullptr, nullptr, nullptr), "NULL"), "NULL inv_metric");
    {
        std::vector<double> b = sig;
        b[5 * 2 + 1] = NAN;
        EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 3, b.data(), &o, nullptr, nullptr, nullptr), "not finite"), "a NaN entry");
        b = sig;
        b[5 * 3 + 3] = -1.0;
        EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 3, b.data(), &o, nullptr, nullptr, nullptr), "> 0"), "a negative diagonal");
        b = sig;
        b[5 * 1 + 0] = 10.0;
        EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 3, b.data(), &o, nullptr, nullptr, nullptr), "positive definite"), "an indefinite matrix");
    }
    EXPECT(refused(lr_run_nuts_dense(m, st.data(), 0.1, 3, sig.data(), nullptr, nullptr, nullptr, nullptr), "NULL"), "NULL opts");
    EXPECT(refused(lr_run_nuts_dense(m, nullptr, 0.1, 3, sig.data(), &o, nullptr, nullptr, nullptr), "NULL"), "NULL state");
    {
        const std::vector<double> w = spd(32);  // (the wide model's own p x p is never read: p > 32 is refused first)
        EXPECT(lr_run_nuts_dense(wide, st.data(), 0.1, 3, w.data(), &o, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "p = 40 > 32"), "a wide model");
    }
    lr_run_opts b = o;
    b.group = 8;
    EXPECT(lr_run_nuts_dense(m, st.data(), 0.1, 3, sig.data(), &b, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "group 8"), "8 lanes per chain");
    b = o;
    b.mode = 4;
    EXPECT(lr_run_nuts_dense(m, st.data(), 0.1, 3, sig.data(), &b, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "stepwise"), "the stepwise engine");
    EXPECT(hipstub_mallocs() == mallocs0 && hipstub_launches() == l0, "refused before any device access");
    {   // the matrices beyond the LDS: the diagonal kernel still fits, the dense one is refused with its own reason
        lr_model* tall = model(LR_F64, 20, 300);
        if (tall) {
            std::vector<double> s2(8 * 20, 0.0), dm(20, 1.0);
            const std::vector<double> sg = spd(20);
            EXPECT(lr_run_nuts(tall, s2.data(), 0.1, 10, dm.data(), &o, nullptr, nullptr, nullptr) == LR_OK, "the diagonal kernel fits (n = 300, p = 20, max_depth 10: 163 520 of 163 840 bytes)");
            EXPECT(lr_run_nuts_dense(tall, s2.data(), 0.1, 10, sg.data(), &o, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "dense metric's two matrices (16384 bytes)"),
                   "the dense kernel does not");
            EXPECT(lr_run_nuts_dense(tall, s2.data(), 0.1, 3, sg.data(), &o, nullptr, nullptr, nullptr) == LR_OK, "... until the checkpoints shrink");
            lr_model_destroy(tall);
        }
    }
    EXPECT(lr_run_nuts_dense(m, st.data(), 0.1, 3, sig.data(), &o, out.data(), cnt.data(), dep.data()) == LR_OK, "after all the refusals");
    lr_model_destroy(m);
    lr_model_destroy(wide);
}

static void warmup(int dtype, int p, int64_t C, int W, int adapt_metric, void* stream) {
    lr_model* m = model(dtype, p);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const std::vector<double> sig = spd(p);
    lr_adapt* h = nullptr;
    lr_adapt_opts ao = adapt_opts(W, adapt_metric, 0.25);
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(lr_dense_adapt_create(m, C, &ao, sig.data(), &h) == LR_OK && h, "create (C %lld, p %d, W %d)", (long long)C, p, W);
    const long in_create = hipstub_mallocs() - m0;
    if (h) {
        double eps = -1;
        std::vector<double> got((size_t)p * p, -1.0);
        lr_adapt_info info;
        EXPECT(lr_dense_adapt_result(h, &eps, got.data(), &info) == LR_OK && eps == 0.25 && got == sig && info.iterations == 0 && info.windows == 0 && info.metric_skipped == 0, "the start values");
        int32_t ends[LR_ADAPT_MAX_WINDOWS], nw = 0, init = 0;
        EXPECT(lr_adapt_schedule(W, 0, 0, 0, ends, &nw, &init) == LR_OK, "schedule");
        if (!adapt_metric) nw = 0;
        EXPECT(info.n_windows == nw, "windows %d, schedule %d", info.n_windows, nw);
        long in_windows = 0;
        for (int w = 0; w < nw; ++w) in_windows += ends[w] - (w ? ends[w - 1] : init);
        std::vector<unsigned char> state(C * p * es, 0), out((size_t)W * C * p * es, 0);
        std::vector<lr_nuts_counters> cnt((size_t)C);
        std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
        std::vector<int8_t> depth((size_t)W * C, 0);
        std::vector<double> astat((size_t)W * C, 0.0);
        lr_run_opts ho = run_opts(C, 0, nullptr, 2), dopt = run_opts(C, 1, stream, 2);
        const long n0 = hipstub_launches(), k0 = hipstub_launches_of("k_nuts_dense"), c0 = hipstub_launches_of("k_dense_comoment"), d0 = hipstub_launches_of("k_nuts<");
        const int64_t first = W > 8 ? 7 : W - 1;
        EXPECT(lr_dense_adapt_run(h, state.data(), 0, 5, &ho, nullptr, nullptr, nullptr, nullptr) == LR_OK, "nothing to do");
        EXPECT(lr_dense_adapt_run(h, state.data(), 1, 5, &ho, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "one iteration, host pointers, every array");
        if (first > 0) EXPECT(lr_dense_adapt_run(h, state.data(), first, 5, &ho, nullptr, nullptr, nullptr, nullptr) == LR_OK, "host pointers, the state alone");
        Dev dstate(C * p * es), dout((size_t)W * C * p * es);
        const int64_t rest = W - 1 - first;
        m0 = hipstub_mallocs();
        if (rest > 0) EXPECT(lr_dense_adapt_run(h, dstate.p, rest, 5, &dopt, dout.p, nullptr, nullptr, nullptr) == LR_OK, "the rest from device memory, across the window ends");
        EXPECT(hipstub_mallocs() == m0, "a run on device pointers allocates nothing (%ld)", hipstub_mallocs() - m0);
        EXPECT(hipstub_launches() - n0 == 3L * W + 2 * in_windows && hipstub_launches_of("k_nuts_dense") - k0 == W && hipstub_launches_of("k_dense_comoment") - c0 == 2 * in_windows &&
                   hipstub_launches_of("k_nuts<") == d0, "%ld launches for %d iterations, %ld of them in windows", hipstub_launches() - n0, W, in_windows);
        EXPECT(lr_dense_adapt_result(h, &eps, got.data(), &info) == LR_OK && info.iterations == W && info.windows == nw && info.metric_skipped == 0, "all %d iterations, %d windows (%lld, %d, %lld skipped)",
               W, nw, (long long)info.iterations, info.windows, (long long)info.metric_skipped);
        // no-op kernels leave the co-moment empty: Sigma = 1e-3 I after a window, the start matrix without one
        EXPECT(nw ? (got[0] == 1e-3 && (p == 1 || got[1] == 0.0)) : got == sig, "the metric after the warm-up");
        std::vector<double> trace((size_t)W * LR_ADAPT_TRACE_COLS, 7.0), metric((size_t)(nw ? nw : 1) * p * p, 7.0);
        EXPECT(lr_dense_adapt_trace(h, trace.data(), metric.data()) == LR_OK && trace[0] != 7.0 && trace.back() != 7.0 && (nw == 0 || (metric[0] == 1e-3 && metric.back() == 1e-3)), "trace and metric are written whole");
        EXPECT(lr_dense_adapt_trace(h, nullptr, nullptr) == LR_OK && lr_dense_adapt_result(h, nullptr, nullptr, nullptr) == LR_OK, "nothing asked");
        auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
        EXPECT(refused(lr_dense_adapt_run(h, state.data(), 1, 5, &ho, nullptr, nullptr, nullptr, nullptr), "remain"), "no iteration is left");
        EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
        lr_dense_adapt_destroy(h);
        h = nullptr;
    }
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the handle", hipstub_live_allocs() - live0);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = lr_dense_adapt_create(m, C, &ao, sig.data(), &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h, "allocation %ld of %ld of create fails: rc %d", k, in_create, rc);
        if (h) lr_dense_adapt_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "allocation %ld of create fails: %ld device buffers leaked", k, hipstub_live_allocs() - live0);
    }
    lr_model_destroy(m);
}

static void warmup_errors() {
    lr_model* m = model(LR_F32, 5);
    if (!m) return;
    const std::vector<double> sig = spd(5);
    lr_adapt* h = nullptr;
    lr_adapt_opts ao = adapt_opts(40, 1, 0.25);
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    const long mallocs0 = hipstub_mallocs();
    EXPECT(refused(lr_dense_adapt_create(nullptr, 8, &ao, sig.data(), &h), "NULL") && refused(lr_dense_adapt_create(m, 8, nullptr, sig.data(), &h), "NULL") &&
               refused(lr_dense_adapt_create(m, 8, &ao, sig.data(), nullptr), "NULL"), "NULL model / opts / out");
    {
        std::vector<double> d(5, 1.0);
        lr_adapt_opts b = ao;
        b.dmm0 = d.data();
        EXPECT(refused(lr_dense_adapt_create(m, 8, &b, sig.data(), &h), "dmm0"), "dmm0 beside a dense metric");
        std::vector<double> bad = sig;
        bad[5 * 4 + 4] = 0.0;
        EXPECT(refused(lr_dense_adapt_create(m, 8, &ao, bad.data(), &h), "> 0"), "a zero diagonal");
        b = ao;
        b.W = 0;
        EXPECT(refused(lr_dense_adapt_create(m, 8, &b, sig.data(), &h), "W must"), "lr_adapt_create's own refusals");
    }
    EXPECT(refused(lr_dense_adapt_create(m, 0, &ao, sig.data(), &h), "positive"), "C");
    EXPECT(h == nullptr && hipstub_mallocs() == mallocs0, "refused before any device access");
    EXPECT(lr_dense_adapt_create(m, 8, &ao, nullptr, &h) == LR_OK && h, "NULL inv_metric is the unit metric");
    if (h) {
        std::vector<double> got(25, -1.0);
        EXPECT(lr_dense_adapt_result(h, nullptr, got.data(), nullptr) == LR_OK && got[0] == 1.0 && got[1] == 0.0 && got[24] == 1.0, "the unit metric");
        lr_dense_adapt_destroy(h);
    }
    h = nullptr;
    EXPECT(lr_adapt_create(m, 8, &ao, &h) == LR_OK && h, "a diagonal handle");
    if (h) {
        std::vector<float> st(8 * 5, 0.f);
        lr_run_opts o = run_opts(8, 0, nullptr, 2);
        EXPECT(refused(lr_dense_adapt_run(h, st.data(), 1, 5, &o, nullptr, nullptr, nullptr, nullptr), "not one of") && refused(lr_dense_adapt_result(h, nullptr, nullptr, nullptr), "not one of") &&
                   refused(lr_dense_adapt_trace(h, nullptr, nullptr), "not one of"), "a diagonal handle is refused by the dense calls");
        lr_adapt_destroy(h);
    }
    EXPECT(refused(lr_dense_adapt_run(nullptr, nullptr, 1, 5, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL") && refused(lr_dense_adapt_result(nullptr, nullptr, nullptr, nullptr), "NULL") &&
               refused(lr_dense_adapt_trace(nullptr, nullptr, nullptr), "NULL"), "NULL handle");
    lr_dense_adapt_destroy(nullptr);
    lr_model_destroy(m);
}

int main() {
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    factor();
    for (int dtype : {LR_F32, LR_F64})
        for (int p : {3, 8, 20}) {
            runs(dtype, p, 37, stream);
            runs(dtype, p, 1025, stream);
            warmup(dtype, p, 37, 60, 1, stream);
            warmup(dtype, p, 1025, 150, 1, stream);
            warmup(dtype, p, 300, 150, 0, stream);
            warmup(dtype, p, 1, 19, 1, stream);
        }
    run_errors();
    warmup_errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("dense harness", "k_nuts_dense");
}
