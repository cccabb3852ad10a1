// pg_harness.cpp -- TEST INFRASTRUCTURE: the host side of the Polya-Gamma Gibbs sampler (include/logreg_hip_pg.h; lr_api.hip, lr_plan.h
// plan_pg) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory is the
// host heap) and compiled with -fsanitize=address,undefined by tests/test_pg_cpu.py, after the pattern of dense_harness.cpp.  It drives
// the C ABI: every refused argument ahead of any device access, the planner's answers and refusals with their reasons, the vector
// b = X^T (y - 1/2) the model carries, lr_run_pg and lr_pg_omega in both dtypes from host and from device memory, and a failing allocation
// at every allocation of a host-pointer call.  With no-op kernels what is checked is the host logic, not arithmetic.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "harness.h"
#include "logreg_hip_pg.h"
#include "lr_model.h"  // struct lr_model: pg_b

static Design g_d;  // the design of the latest model: the_vector_b reads it
static lr_model* pg_model(int dtype, int p, int64_t n = 50) { return model(dtype, p, n, 1.5, true, &g_d); }

static bool refused(int rc, int code, const char* word) { return rc == code && std::strstr(lr_last_error(), word) != nullptr; }

static void the_vector_b() {
    for (int dtype : {LR_F32, LR_F64})
        for (int p : {1, 3, 8, 20, 32}) {
            lr_model* m = pg_model(dtype, p, 37);
            if (!m) continue;
            EXPECT((int)m->pg_b.size() == p, "b has p entries");
            for (int j = 0; j < p && j < (int)m->pg_b.size(); ++j) {
                double want = 0;  // X^T (y - 1/2) of the rows as stored
                for (int64_t i = 0; i < 37; ++i) {
                    const double x = dtype == LR_F32 ? (double)(float)g_d.X[i * p + j] : g_d.X[i * p + j];
                    want += (g_d.y[i] - 0.5) * x;
                }
                EXPECT(std::fabs(m->pg_b[j] - want) <= 1e-13 * (1.0 + std::fabs(want)), "b[%d] = %.17g, X^T (y - 1/2) = %.17g (dtype %d, p %d)", j, m->pg_b[j], want, dtype, p);
            }
            lr_model_destroy(m);
        }
}

static void planner() {
    lr_model* m = pg_model(LR_F32, 8, 200);
    lr_run_opts o = run_opts(4096, 1, nullptr, 2);
    lr_plan_info pi;
    EXPECT(lr_plan_run_info(m, LR_KIND_PG, &o, &pi) == LR_OK && pi.mode == LR_MODE_LDS && pi.group == 16 && pi.split == 0, "Pima's shape plans as lds, 16 lanes");
    int32_t mode = -7, group = -7, rows = -7;
    EXPECT(lr_plan_run(m, LR_KIND_PG, &o, &mode, &group, &rows) == LR_OK && mode == LR_MODE_LDS && group == 16 && rows == 0, "lr_plan_run");
    EXPECT(refused(lr_plan_run_info(m, 5, &o, &pi), LR_ERR_INVALID, "LR_KIND"), "kind 5 is not a kind of the ABI");
    EXPECT(refused(lr_plan_run_info(m, 7, &o, &pi), LR_ERR_INVALID, "LR_KIND"), "kind 7");
    o.group = 16;
    o.mode = LR_MODE_LDS;
    EXPECT(lr_plan_run_info(m, LR_KIND_PG, &o, &pi) == LR_OK, "the family's own mode and group may be named");
    o.group = 8;
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "16 lanes per chain only"), "group 8");
    o.group = 0;
    o.mode = LR_MODE_REG;
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "rows in LDS only"), "mode reg");
    lr_model_destroy(m);
    o = run_opts(64, 1, nullptr, 2);
    m = pg_model(LR_F32, 40, 30);
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "p = 40 > 32"), "p = 40");
    lr_model_destroy(m);
    m = pg_model(LR_F32, 8, 20000);
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "bytes of LDS"), "n = 20 000 at p = 8: rows beyond the LDS");
    lr_model_destroy(m);
    m = pg_model(LR_F32, 2, 65536);
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "n = 65536 >= 65536"), "n = 65 536");
    lr_model_destroy(m);
    // the LDS arithmetic: float64 p = 8 pads a row to 10 doubles; rows + 16 n doubles of staging
    m = pg_model(LR_F64, 8, 787);  // 787 * (80 + 128) = 163 696 <= 163 840
    EXPECT(lr_plan_run_info(m, LR_KIND_PG, &o, &pi) == LR_OK, "787 float64 rows of 8 fit");
    lr_model_destroy(m);
    m = pg_model(LR_F64, 8, 788);  // 163 904
    EXPECT(refused(lr_plan_run_info(m, LR_KIND_PG, &o, &pi), LR_ERR_UNSUPPORTED, "163904 bytes of LDS"), "788 do not");
    lr_model_destroy(m);
}

static void runs() {
    for (int dtype : {LR_F32, LR_F64})
        for (int p : {3, 8, 20, 32}) {
            lr_model* m = pg_model(dtype, p);
            if (!m) continue;
            const int64_t C = 37, n = 50, iters = 3;
            const size_t es = dtype == LR_F32 ? 4 : 8;
            std::vector<unsigned char> state(C * p * es, 0), out(iters * C * p * es, 0), omega(C * n * es, 0);
            std::vector<lr_pg_counters> cn((size_t)C);
            std::memset(cn.data(), 0, cn.size() * sizeof(lr_pg_counters));
            std::vector<double> stats((size_t)2 * C * 2 * p, 0.0);
            lr_run_opts o = run_opts(C, 0, nullptr, iters);
            // refusals, ahead of any device access
            const long m0 = hipstub_mallocs(), l0 = hipstub_launches();
            EXPECT(refused(lr_run_pg(nullptr, state.data(), &o, nullptr, nullptr), LR_ERR_INVALID, "model is NULL"), "no model");
            EXPECT(refused(lr_run_pg(m, nullptr, &o, nullptr, nullptr), LR_ERR_INVALID, "state is NULL"), "no state");
            EXPECT(refused(lr_run_pg(m, state.data(), nullptr, nullptr, nullptr), LR_ERR_INVALID, "opts is NULL"), "no opts");
            EXPECT(refused(lr_pg_omega(m, state.data(), &o, nullptr), LR_ERR_INVALID, "omega_out is NULL"), "no omega_out");
            EXPECT(refused(lr_pg_omega(m, nullptr, &o, omega.data()), LR_ERR_INVALID, "state is NULL"), "omega: no state");
            EXPECT(refused(lr_pg_omega(nullptr, state.data(), &o, omega.data()), LR_ERR_INVALID, "model is NULL"), "omega: no model");
            lr_run_opts bad = o;
            bad.n_chains = 0;
            EXPECT(refused(lr_run_pg(m, state.data(), &bad, nullptr, nullptr), LR_ERR_INVALID, "n_chains"), "no chains");
            bad = o;
            bad.thin = 0;
            EXPECT(refused(lr_run_pg(m, state.data(), &bad, nullptr, nullptr), LR_ERR_INVALID, "thin"), "thin 0");
            EXPECT(lr_pg_omega(m, state.data(), &bad, omega.data()) == LR_OK, "lr_pg_omega does not read thin");
            bad = o;
            bad.group = 4;
            EXPECT(refused(lr_run_pg(m, state.data(), &bad, nullptr, nullptr), LR_ERR_UNSUPPORTED, "16 lanes"), "group 4");
            bad = o;
            bad.stats = stats.data();
            bad.stats_batch = 1;
            bad.stats_slots = 2;  // 3 kept samples need 3 slots
            EXPECT(refused(lr_run_pg(m, state.data(), &bad, nullptr, nullptr), LR_ERR_INVALID, "stats buffer too small"), "statistics window");
            EXPECT(hipstub_mallocs() == m0 + 2 && hipstub_launches() == l0 + 1, "refusals come ahead of any device access (two allocations, one launch: the omega call that was valid)");
            // host pointers: with and without the optional arrays
            const long k0 = hipstub_launches_of("k_pg"), a0 = hipstub_live_allocs();
            EXPECT(lr_run_pg(m, state.data(), &o, out.data(), cn.data()) == LR_OK, "host run (dtype %d, p %d)", dtype, p);
            EXPECT(lr_run_pg(m, state.data(), &o, nullptr, nullptr) == LR_OK, "host run, no out, no counters");
            lr_run_opts so = o;
            so.stats = stats.data();
            so.stats_batch = 2;
            so.stats_slots = 2;
            EXPECT(lr_run_pg(m, state.data(), &so, nullptr, cn.data()) == LR_OK, "host run with streaming statistics");
            EXPECT(lr_pg_omega(m, state.data(), &o, omega.data()) == LR_OK, "host omega");
            lr_run_opts none = o;
            none.iters = 0;
            EXPECT(lr_run_pg(m, state.data(), &none, nullptr, nullptr) == LR_OK, "nothing to do");
            EXPECT(hipstub_launches_of("k_pg") == k0 + 4, "one launch per call that runs: %ld", hipstub_launches_of("k_pg") - k0);
            EXPECT(hipstub_live_allocs() == a0, "staging freed");
            // a failing allocation at every allocation of a host-pointer call
            for (long nth = 1; nth <= 3; ++nth) {  // state, out, counters
                int rc;
                { FailMallocAt failing(nth); rc = lr_run_pg(m, state.data(), &o, out.data(), cn.data()); }
                EXPECT(refused(rc, LR_ERR_NOMEM, "device allocation failed"), "allocation %ld fails: rc %d", nth, rc);
                EXPECT(hipstub_live_allocs() == a0, "nothing leaks after allocation %ld failed", nth);
            }
            // device pointers
            {
                Dev ds(state.size()), dout(out.size()), dcn(cn.size() * sizeof(lr_pg_counters)), dom(omega.size());
                lr_run_opts od = run_opts(C, 1, nullptr, iters);
                od.chain_offset = 1000;
                od.iter_offset = 77;
                const long k1 = hipstub_launches_of("k_pg");
                EXPECT(lr_run_pg(m, ds.p, &od, dout.p, static_cast<lr_pg_counters*>(dcn.p)) == LR_OK, "device run");
                EXPECT(lr_pg_omega(m, ds.p, &od, dom.p) == LR_OK, "device omega");
                EXPECT(hipstub_launches_of("k_pg") == k1 + 2, "two launches");
            }
            EXPECT(hipstub_live_allocs() == a0, "device buffers freed");
            lr_model_destroy(m);
        }
}

int main() {
    the_vector_b();
    planner();
    runs();
    return finish("pg harness", nullptr);
}
