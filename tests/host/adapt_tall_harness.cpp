// adapt_tall_harness.cpp -- TEST INFRASTRUCTURE: the host side of the NUTS warm-up on the stepwise engine (include/logreg_hip_adapt_tall.h;
// lr_api.hip, lr_engine.h) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device
// memory is the host heap) and compiled with -fsanitize=address,undefined by tests/test_adapt_tall_cpu.py.  It checks which shapes
// lr_tall_adapt_create takes, every refusal of lr_tall_adapt_run ahead of any device access, a failing device allocation at EVERY
// allocation of a run, the launches booked per iteration and per call, and that an iteration ends after 2^max_depth - 1 leaves under a
// tally that never reaches zero.  With no-op kernels the tally of building chains reads zero: an iteration then ends at the first read.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lr_model.h"  // (the model handle: its stepwise workspace is filled by hand for the tally that never reaches zero)
#include "logreg_hip_adapt_tall.h"
#include "harness.h"

static lr_run_opts stepwise_opts(int64_t C) { return run_opts(C, 0, nullptr, 1, LR_MODE_STEPWISE); }

struct Counts {
    long all, update, load, apart, aupd, partial = 0;
    static Counts now() {
        // (names as the code objects register them, mangled.  k_tall_updateI: the engine's load; `partial` is set by operator-: whatever is
        // none of the others is an evaluation, whose kernel differs by width and dtype.  The adaptation kernels are k_adapt_* up to P = 32
        // and k_tall_adapt_* beyond)
        return {hipstub_launches(), hipstub_launches_of("k_tall_nuts_update"), hipstub_launches_of("k_tall_updateI"),
                hipstub_launches_of("k_adapt_partial") + hipstub_launches_of("k_tall_adapt_partial"), hipstub_launches_of("k_adapt_update") + hipstub_launches_of("k_tall_adapt_update")};
    }
    Counts operator-(const Counts& o) const {
        Counts d{all - o.all, update - o.update, load - o.load, apart - o.apart, aupd - o.aupd};
        d.partial = d.all - d.update - d.load - d.apart - d.aupd;
        return d;
    }
};

static void shapes() {
    lr_adapt_opts ao = adapt_opts(40);
    lr_adapt* h = nullptr;
    lr_model* fused = model(LR_F32, 4, 50);
    const long mallocs0 = hipstub_mallocs();
    EXPECT(lr_tall_adapt_create(fused, 8, &ao, &h) == LR_ERR_UNSUPPORTED && !h && std::strstr(lr_last_error(), "lr_adapt_create") != nullptr, "a shape of the fused kernel, with the hint");
    EXPECT(lr_tall_adapt_create(nullptr, 8, &ao, &h) == LR_ERR_INVALID && lr_tall_adapt_create(fused, 0, &ao, &h) == LR_ERR_INVALID && std::strstr(lr_last_error(), "lr_tall_adapt_create: C") != nullptr,
           "lr_adapt_create's argument checks under this entry point's name");
    EXPECT(hipstub_mallocs() == mallocs0, "refused before any device access");
    lr_model_destroy(fused);
    for (int which = 0; which < 2; ++which) {
        lr_model* m = which == 0 ? model(LR_F32, 40, 64) : model(LR_F64, 20, 1200);  // wide; narrow with rows beyond the LDS
        const int p = which == 0 ? 40 : 20;
        EXPECT(lr_tall_adapt_create(m, 8, &ao, &h) == LR_OK && h, "create (%s)", which == 0 ? "p = 40" : "rows beyond the LDS");
        if (h) {
            std::vector<double> state((size_t)8 * p, 0.0), stats(4096, 0.0);
            lr_run_opts o = stepwise_opts(8);
            const long l0 = hipstub_launches(), m0 = hipstub_mallocs();
            lr_run_opts b = o;
            b.mode = LR_MODE_AUTO;
            EXPECT(lr_tall_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "LR_MODE_STEPWISE") != nullptr, "another mode");
            b = o;
            b.stats = stats.data();
            EXPECT(lr_tall_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "stats") != nullptr, "streaming statistics");
            EXPECT(lr_tall_adapt_run(h, state.data(), 41, 5, &o, nullptr, nullptr, nullptr, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "remain") != nullptr, "iters beyond what remains");
            b = o;
            b.n_chains = 7;
            EXPECT(lr_tall_adapt_run(h, state.data(), 1, 5, &b, nullptr, nullptr, nullptr, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "n_chains") != nullptr, "another chain count");
            EXPECT(lr_adapt_run(h, state.data(), 1, 5, &o, nullptr, nullptr, nullptr, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "lr_tall_adapt_run") != nullptr, "lr_adapt_run on this handle");
            EXPECT(hipstub_launches() == l0 && hipstub_mallocs() == m0, "refused before any device access");
            lr_adapt_destroy(h);
            h = nullptr;
        }
        lr_model_destroy(m);
    }
    lr_model* narrow = model(LR_F32, 5, 50);
    EXPECT(lr_adapt_create(narrow, 8, &ao, &h) == LR_OK && h, "a fused handle");
    if (h) {
        std::vector<float> st(8 * 5, 0.f);
        lr_run_opts o = stepwise_opts(8);
        EXPECT(lr_tall_adapt_run(h, st.data(), 1, 5, &o, nullptr, nullptr, nullptr, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "lr_tall_adapt_create") != nullptr, "a fused handle is refused");
        lr_adapt_destroy(h);
    }
    lr_model_destroy(narrow);
}

// the launches of a call of `iters` iterations at max_depth md under a tally that reads `tally` at every doubling
static void launches(int dtype, int p, int64_t n, int64_t C, int md, bool never_zero) {
    lr_model* m = model(dtype, p, n);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int W = 30;
    lr_adapt_opts ao = adapt_opts(W);
    lr_adapt* h = nullptr;
    EXPECT(lr_tall_adapt_create(m, C, &ao, &h) == LR_OK && h, "create");
    std::vector<unsigned char> state((size_t)C * p * es, 0), out((size_t)W * C * p * es, 0);
    std::vector<lr_nuts_counters> cnt((size_t)C);
    std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
    std::vector<int8_t> depth((size_t)W * C, 0);
    std::vector<double> astat((size_t)W * C, 0.0);
    lr_run_opts o = stepwise_opts(C);
    EXPECT(lr_tall_adapt_run(h, state.data(), 1, md, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "a first call (it allocates the workspace)");
    if (never_zero)  // no-op kernels never write the tally: every read of it gives 0xFFFFFFFF chains still building
        for (auto& w : m->ws) std::memset(w.p, 0xFF, w.bytes);
    // leaves of an iteration: all 2^md - 1 under a tally that stays positive; with a zero tally the first doubling's one leaf (md = 1: no read)
    const long leaves = never_zero ? (1L << md) - 1 : 1;
    const Counts c0 = Counts::now();
    const int64_t iters = 7;
    EXPECT(lr_tall_adapt_run(h, state.data(), iters, md, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "%lld iterations", (long long)iters);
    const Counts d = Counts::now() - c0;
    // per call: load (k_tall_update), the evaluation at x, begin ... store; per iteration: per leaf an evaluation and a leaf update, end,
    // partial, update; from the second iteration on a begin of its own
    EXPECT(d.partial == 1 + iters * leaves, "evaluations: %ld, expected %ld", d.partial, 1 + iters * leaves);
    EXPECT(d.update == 1 + (iters - 1) + iters * leaves + iters + 1, "k_tall_nuts_update launches: %ld, expected %ld (begin, %lld carried begins, leaves, ends, store)", d.update,
           1 + (iters - 1) + iters * leaves + iters + 1, (long long)(iters - 1));
    EXPECT(d.apart == iters && d.aupd == iters, "adaptation launches: %ld partial, %ld update for %lld iterations", d.apart, d.aupd, (long long)iters);
    EXPECT(d.load == 1, "%ld loads in one call", d.load);
    lr_adapt_info info;
    EXPECT(lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK && info.iterations == 1 + iters, "the iterations are counted (%lld)", (long long)info.iterations);
    std::vector<double> trace((size_t)W * LR_ADAPT_TRACE_COLS, 7.0);
    EXPECT(lr_adapt_trace(h, trace.data(), nullptr) == LR_OK && trace[0] != 7.0, "the trace reads as before");
    lr_adapt_destroy(h);
    lr_model_destroy(m);
}

static void failing_allocations(int dtype, int p, int64_t n, int64_t C) {
    lr_model* m = model(dtype, p, n);
    if (!m) return;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int W = 30;
    lr_adapt_opts ao = adapt_opts(W);
    lr_adapt* h = nullptr;
    lr_adapt_info info;
    std::vector<unsigned char> state((size_t)C * p * es, 0), out((size_t)W * C * p * es, 0);
    std::vector<lr_nuts_counters> cnt((size_t)C);
    std::memset(cnt.data(), 0, cnt.size() * sizeof(lr_nuts_counters));
    std::vector<int8_t> depth((size_t)W * C, 0);
    std::vector<double> astat((size_t)W * C, 0.0);
    lr_run_opts o = stepwise_opts(C);
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(lr_tall_adapt_create(m, C, &ao, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    lr_adapt_destroy(h);
    h = nullptr;
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = lr_tall_adapt_create(m, C, &ao, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h && hipstub_live_allocs() == live0, "allocation %ld of create fails: rc %d", k, rc);
    }
    // a run with host pointers allocates five staging buffers and, the first time on a model, the engine's workspace; a longer run grows them
    for (int regrow = 0; regrow < 2; ++regrow) {
        EXPECT(lr_tall_adapt_create(m, C, &ao, &h) == LR_OK && h, "fresh");
        if (regrow) EXPECT(lr_tall_adapt_run(h, state.data(), 2, 4, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "run");
        m0 = hipstub_mallocs();
        EXPECT(lr_tall_adapt_run(h, state.data(), 9, regrow ? 6 : 4, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "the run whose allocations are counted");
        const long in_run = hipstub_mallocs() - m0;
        lr_adapt_destroy(h);
        h = nullptr;
        EXPECT(in_run >= (regrow ? 3 : 5), "allocations of a run: %ld", in_run);
        for (long k = 1; k <= in_run; ++k) {
            lr_model* mm = model(dtype, p, n);  // (a model of its own: the workspace lives with the model)
            EXPECT(lr_tall_adapt_create(mm, C, &ao, &h) == LR_OK && h, "fresh");
            if (regrow) EXPECT(lr_tall_adapt_run(h, state.data(), 2, 4, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK, "run");
            const int64_t before = regrow ? 2 : 0;
            const long l0 = hipstub_launches();
            int rc;
            { FailMallocAt failing(k); rc = lr_tall_adapt_run(h, state.data(), 9, regrow ? 6 : 4, &o, out.data(), cnt.data(), depth.data(), astat.data()); }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == l0, "allocation %ld of %ld of a run fails (regrow %d): rc %d, %ld launches", k, in_run, regrow, rc, hipstub_launches() - l0);
            EXPECT(lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK && info.iterations == before, "the count stays %lld after a failed run (%lld)", (long long)before, (long long)info.iterations);
            EXPECT(lr_tall_adapt_run(h, state.data(), 9, regrow ? 6 : 4, &o, out.data(), cnt.data(), depth.data(), astat.data()) == LR_OK && lr_adapt_result(h, nullptr, nullptr, &info) == LR_OK &&
                       info.iterations == before + 9, "usable after a failed run");
            lr_adapt_destroy(h);
            h = nullptr;
            lr_model_destroy(mm);
        }
    }
    lr_model_destroy(m);
    EXPECT(hipstub_live_allocs() <= live0, "%ld device buffers leaked", hipstub_live_allocs() - live0);
}

int main() {
    shapes();
    for (int md : {1, 2, 4, 6}) {
        launches(LR_F32, 40, 64, 37, md, false);
        launches(LR_F32, 40, 64, 37, md, true);
        launches(LR_F64, 100, 64, 300, md, true);   // P = 128, two workgroups of the partial kernel
        launches(LR_F64, 20, 1200, 5, md, true);    // narrow, rows beyond the LDS
    }
    failing_allocations(LR_F32, 40, 64, 300);
    failing_allocations(LR_F64, 20, 1200, 9);
    return finish("adapt tall harness", "k_tall_nuts_update");
}
