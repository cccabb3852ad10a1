// hs_harness.cpp -- TEST INFRASTRUCTURE: the host side of the horseshoe Polya-Gamma Gibbs sampler (include/logreg_hip_hs.h; lr_api.hip) as
// a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory is the host heap) and
// compiled with -fsanitize=address,undefined by tests/test_hs_cpu.py, after the pattern of pg_harness.cpp.  It drives the C ABI: every
// refused argument ahead of any device access, the planner's refusals (lr_run_pg's), lr_run_hs and lr_hs_hyper in both dtypes from host and
// from device memory with and without the optional arrays, and a failing allocation at every allocation of a host-pointer call.  With
// no-op kernels what is checked is the host logic, not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "harness.h"
#include "logreg_hip_hs.h"

static bool refused(int rc, int code, const char* word) { return rc == code && std::strstr(lr_last_error(), word) != nullptr; }

static void runs() {
    for (int dtype : {LR_F32, LR_F64})
        for (int p : {3, 8, 20, 32}) {
            lr_model* m = model(dtype, p, 50, 1.5, true);
            if (!m) continue;
            const int64_t C = 37, iters = 3;
            const size_t es = dtype == LR_F32 ? 4 : 8, hw = 2 * (size_t)p + 2;
            std::vector<unsigned char> state(C * p * es, 0), out(iters * C * p * es, 0);
            std::vector<double> hyper(C * hw, 1.0), hyper2(C * hw, 0.0), scales(iters * C * (p + 1), 0.0), stats((size_t)2 * C * 2 * p, 0.0);
            std::vector<lr_hs_counters> cn((size_t)C);
            std::memset(cn.data(), 0, cn.size() * sizeof(lr_hs_counters));
            std::vector<uint8_t> mask((size_t)p, 1), none((size_t)p, 0);
            mask[0] = 0;
            const lr_hs_prior pr{mask.data(), 0.5};
            lr_run_opts o = run_opts(C, 0, nullptr, iters);
            // refusals, ahead of any device access
            const long m0 = hipstub_mallocs(), l0 = hipstub_launches();
            EXPECT(refused(lr_run_hs(nullptr, &pr, state.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "model is NULL"), "no model");
            EXPECT(refused(lr_run_hs(m, nullptr, state.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "prior is NULL"), "no prior");
            lr_hs_prior bad_pr{nullptr, 0.5};
            EXPECT(refused(lr_run_hs(m, &bad_pr, state.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "shrink is NULL"), "no mask");
            for (double gs : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
                bad_pr = lr_hs_prior{mask.data(), gs};
                EXPECT(refused(lr_run_hs(m, &bad_pr, state.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "global_scale"), "global_scale %g", gs);
                EXPECT(refused(lr_hs_hyper(m, &bad_pr, state.data(), hyper.data(), &o, hyper2.data(), nullptr), LR_ERR_INVALID, "global_scale"), "hyper: global_scale %g", gs);
            }
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), nullptr, &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "hyper is NULL"), "no hyper");
            for (double v : {0.0, -2.0, 1e-101, 1e101, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
                std::vector<double> h = hyper;
                h[(size_t)(C - 1) * hw + hw - 1] = v;
                EXPECT(refused(lr_run_hs(m, &pr, state.data(), h.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "must be finite and > 0"), "hyper entry %g", v);
                EXPECT(refused(lr_hs_hyper(m, &pr, state.data(), h.data(), &o, hyper2.data(), nullptr), LR_ERR_INVALID, "hyper_in[36]"), "hyper_in entry %g", v);
            }
            EXPECT(refused(lr_run_hs(m, &pr, nullptr, hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_INVALID, "state is NULL"), "no state");
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), hyper.data(), nullptr, nullptr, nullptr, nullptr), LR_ERR_INVALID, "opts is NULL"), "no opts");
            EXPECT(refused(lr_hs_hyper(m, &pr, state.data(), hyper.data(), nullptr, hyper2.data(), nullptr), LR_ERR_INVALID, "opts is NULL"), "hyper: no opts");
            EXPECT(refused(lr_hs_hyper(m, &pr, state.data(), hyper.data(), &o, nullptr, nullptr), LR_ERR_INVALID, "hyper_out is NULL"), "no hyper_out");
            EXPECT(refused(lr_hs_hyper(m, &pr, state.data(), nullptr, &o, hyper2.data(), nullptr), LR_ERR_INVALID, "hyper_in is NULL"), "no hyper_in");
            EXPECT(refused(lr_hs_hyper(m, &pr, nullptr, hyper.data(), &o, hyper2.data(), nullptr), LR_ERR_INVALID, "state is NULL"), "hyper: no state");
            lr_run_opts bad = o;
            bad.n_chains = 0;
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), hyper.data(), &bad, nullptr, nullptr, nullptr), LR_ERR_INVALID, "n_chains"), "no chains");
            bad = o;
            bad.thin = 0;
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), hyper.data(), &bad, nullptr, nullptr, nullptr), LR_ERR_INVALID, "thin"), "thin 0");
            bad = o;
            bad.group = 4;
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), hyper.data(), &bad, nullptr, nullptr, nullptr), LR_ERR_UNSUPPORTED, "16 lanes"), "group 4: lr_run_pg's planner");
            bad = o;
            bad.stats = stats.data();
            bad.stats_batch = 1;
            bad.stats_slots = 2;  // 3 kept samples need 3 slots
            EXPECT(refused(lr_run_hs(m, &pr, state.data(), hyper.data(), &bad, nullptr, nullptr, nullptr), LR_ERR_INVALID, "stats buffer too small"), "statistics window");
            EXPECT(hipstub_mallocs() == m0 && hipstub_launches() == l0, "refusals come ahead of any device access");
            // host pointers: with and without the optional arrays
            const long k0 = hipstub_launches_of("k_hs"), g0 = hipstub_launches_of("k_pg"), a0 = hipstub_live_allocs();
            EXPECT(lr_run_hs(m, &pr, state.data(), hyper.data(), &o, out.data(), scales.data(), cn.data()) == LR_OK, "host run (dtype %d, p %d)", dtype, p);
            EXPECT(lr_run_hs(m, &pr, state.data(), hyper.data(), &o, nullptr, nullptr, nullptr) == LR_OK, "host run, no out, no scales, no counters");
            lr_run_opts so = o;
            so.stats = stats.data();
            so.stats_batch = 2;
            so.stats_slots = 2;
            EXPECT(lr_run_hs(m, &pr, state.data(), hyper.data(), &so, nullptr, nullptr, cn.data()) == LR_OK, "host run with streaming statistics");
            const lr_hs_prior empty{none.data(), 1.0};
            EXPECT(lr_run_hs(m, &empty, state.data(), hyper.data(), &o, out.data(), nullptr, nullptr) == LR_OK, "the empty set is accepted");
            EXPECT(lr_hs_hyper(m, &pr, state.data(), hyper.data(), &o, hyper2.data(), cn.data()) == LR_OK, "host hyper-step");
            bad = o;
            bad.thin = 0;
            EXPECT(lr_hs_hyper(m, &pr, state.data(), hyper.data(), &bad, hyper2.data(), nullptr) == LR_OK, "lr_hs_hyper does not read thin");
            lr_run_opts zero = o;
            zero.iters = 0;
            EXPECT(lr_run_hs(m, &pr, state.data(), hyper.data(), &zero, nullptr, nullptr, nullptr) == LR_OK, "nothing to do");
            EXPECT(hipstub_launches_of("k_hs") == k0 + 6 && hipstub_launches_of("k_pg") == g0, "one k_hs launch per call that runs: %ld", hipstub_launches_of("k_hs") - k0);
            EXPECT(hipstub_live_allocs() == a0, "staging freed");
            // a failing allocation at every allocation of a host-pointer call
            for (long nth = 1; nth <= 5; ++nth) {  // state, out, counters, hyper, scale_out
                int rc;
                { FailMallocAt failing(nth); rc = lr_run_hs(m, &pr, state.data(), hyper.data(), &o, out.data(), scales.data(), cn.data()); }
                EXPECT(refused(rc, LR_ERR_NOMEM, "device allocation failed"), "allocation %ld fails: rc %d", nth, rc);
                EXPECT(hipstub_live_allocs() == a0, "nothing leaks after allocation %ld failed", nth);
            }
            for (long nth = 1; nth <= 4; ++nth) {  // state, hyper_in, hyper_out, counters
                int rc;
                { FailMallocAt failing(nth); rc = lr_hs_hyper(m, &pr, state.data(), hyper.data(), &o, hyper2.data(), cn.data()); }
                EXPECT(refused(rc, LR_ERR_NOMEM, "device allocation failed"), "hyper-step: allocation %ld fails: rc %d", nth, rc);
                EXPECT(hipstub_live_allocs() == a0, "nothing leaks after allocation %ld of the hyper-step failed", nth);
            }
            // device pointers: the hyper-state is not read on the host
            {
                Dev ds(state.size()), dout(out.size()), dcn(cn.size() * sizeof(lr_hs_counters)), dh(hyper.size() * 8), dh2(hyper.size() * 8), dsc(scales.size() * 8);
                std::memset(dh.p, 0, hyper.size() * 8);  // zeros: refused from host memory, read as LR_HS_MIN by the kernel
                lr_run_opts od = run_opts(C, 1, nullptr, iters);
                od.chain_offset = 1000;
                od.iter_offset = 77;
                const long k1 = hipstub_launches_of("k_hs");
                EXPECT(lr_run_hs(m, &pr, ds.p, static_cast<double*>(dh.p), &od, dout.p, static_cast<double*>(dsc.p), static_cast<lr_hs_counters*>(dcn.p)) == LR_OK, "device run");
                EXPECT(lr_hs_hyper(m, &pr, ds.p, static_cast<double*>(dh.p), &od, static_cast<double*>(dh2.p), nullptr) == LR_OK, "device hyper-step");
                EXPECT(hipstub_launches_of("k_hs") == k1 + 2, "two launches");
            }
            EXPECT(hipstub_live_allocs() == a0, "device buffers freed");
            lr_model_destroy(m);
        }
    // the planner's refusals are lr_run_pg's
    lr_model* m = model(LR_F32, 40, 30);
    std::vector<uint8_t> mask(40, 1);
    std::vector<double> hyper(64 * 82, 1.0);
    std::vector<float> st(64 * 40, 0.f);
    const lr_hs_prior pr{mask.data(), 1.0};
    lr_run_opts o = run_opts(64, 0, nullptr, 2);
    EXPECT(refused(lr_run_hs(m, &pr, st.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_UNSUPPORTED, "p = 40 > 32"), "p = 40");
    lr_model_destroy(m);
    m = model(LR_F32, 8, 20000);
    EXPECT(refused(lr_run_hs(m, &pr, st.data(), hyper.data(), &o, nullptr, nullptr, nullptr), LR_ERR_UNSUPPORTED, "bytes of LDS"), "n = 20 000 at p = 8: rows beyond the LDS");
    lr_model_destroy(m);
}

int main() {
    runs();
    return finish("hs harness", nullptr);
}
