// bridge_harness.cpp -- TEST INFRASTRUCTURE: the host side of the bridge-sampling accumulator (include/logreg_hip_bridge.h; lr_api.hip over
// csrc/lr_accum.h) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory
// is the host heap) and built under the sanitizers by tests/host_build.py.  It drives the C ABI: both dtypes, a padded (5 -> 8, 100 -> 128)
// and an unpadded (8) p, more rows than a slice, host and device input on a stream, terms, proposal draws, result, reset, lr_bridge_solve
// from host and device memory, every refused argument, and a failing device allocation at EVERY allocation of create, accumulate (first
// use and regrow) and solve: LR_ERR_NOMEM, the count unchanged, nothing leaked, the handle usable afterwards.  With no-op kernels the
// terms hold the zeros the stub's allocator fills in: what is checked is the host logic (workspace sizes, chunking, the launch sequence,
// every error path), not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"
#include "logreg_hip_bridge.h"

struct Shape {
    int dtype, p;
    int64_t n;
    size_t draw() const { return (size_t)p * (dtype == LR_F32 ? 4 : 8); }
};

static std::vector<double> spd(int p) {  // 2 I + 0.5 everywhere: positive definite
    std::vector<double> c((size_t)p * p, 0.5);
    for (int i = 0; i < p; ++i) c[(size_t)i * p + i] = 2.5;
    return c;
}

static int create(lr_model* m, int p, int64_t cap, int64_t n2, lr_bridge** h) {
    const std::vector<double> mu((size_t)p, 0.25), cov = spd(p);
    return lr_bridge_create(m, mu.data(), cov.data(), cap, n2, 7, h);
}

static int result(lr_bridge* h, double* t) {
    for (int r = 0; r < LR_BRIDGE_ROWS; ++r) t[r] = 7.0;
    return lr_bridge_result(h, 0.0, 1e-10, 50, t);
}

static void life(const Shape& s, const void* zeros, void* stream) {
    lr_model* m = model(s.dtype, s.p, s.n);
    lr_bridge* h = nullptr;
    double t[LR_BRIDGE_ROWS];
    int64_t n1 = -1, n2 = -1;
    const long p0 = hipstub_launches_of("k_bridge_propose"), f0 = hipstub_launches_of("k_bridge_fill"), g0 = hipstub_launches_of("k_bridge_gauss");
    EXPECT(create(m, s.p, 100, 70, &h) == LR_OK && h, "create (p %d, n %lld)", s.p, (long long)s.n);
    if (!h) return;
    EXPECT(hipstub_launches_of("k_bridge_propose") == p0 + 1 && hipstub_launches_of("k_bridge_fill") == f0 + 1 && hipstub_launches_of("k_bridge_gauss") == g0 + 1,
           "the proposal terms: one launch of each kernel");
    EXPECT(result(h, t) == LR_OK && std::isnan(t[0]) && std::isnan(t[1]) && t[2] == 0 && t[4] == 0 && t[5] == 70, "NaN before the first draw");
    Dev dev(7 * s.draw());
    EXPECT(dev.p != nullptr, "device input");
    const long l0 = hipstub_launches_on(stream);
    EXPECT(lr_bridge_accumulate(h, zeros, 5, 0, stream) == LR_OK, "host input");
    EXPECT(lr_bridge_accumulate(h, dev.p, 7, 1, stream) == LR_OK, "device input");
    EXPECT(hipstub_launches_of("k_bridge_fill") == f0 + 3 && hipstub_launches_of("k_bridge_gauss") == g0 + 3 && hipstub_launches_on(stream) >= l0 + 4,
           "one chunk each, on the caller's stream");
    std::vector<double> l1(12, 7.0), l2(70, 7.0);
    EXPECT(lr_bridge_terms(h, l1.data(), l2.data(), &n1, &n2) == LR_OK && n1 == 12 && n2 == 70 && l1[11] != 7.0 && l2[69] != 7.0, "terms (n1 %lld)", (long long)n1);
    EXPECT(lr_bridge_terms(h, nullptr, nullptr, nullptr, nullptr) == LR_OK, "nothing asked");
    std::vector<unsigned char> prop(70 * s.draw(), 7);
    n2 = -1;
    EXPECT(lr_bridge_proposal(h, prop.data(), &n2) == LR_OK && n2 == 70 && hipstub_launches_of("k_bridge_propose") == p0 + 2, "proposal draws");
    EXPECT(lr_bridge_proposal(h, nullptr, &n2) == LR_OK && hipstub_launches_of("k_bridge_propose") == p0 + 2, "the count alone");
    const long i0 = hipstub_launches_of("k_bridge_iterate");
    EXPECT(result(h, t) == LR_OK && t[4] == 12 && t[5] == 70 && t[6] == 12 && t[7] == 0 && t[2] >= 1, "result of 12 (N1 %g, iterations %g)", t[4], t[2]);
    EXPECT(hipstub_launches_of("k_bridge_iterate") == i0 + 3 + (long)t[2] && hipstub_launches_of("k_bridge_finish") >= 4, "scan, start, %g iterations, error", t[2]);
    EXPECT(lr_bridge_result(h, 5.0, 1e-10, 0, t) == LR_OK && t[6] == 5 && t[2] == 0 && t[3] == 0, "n_eff given, no iteration");
    EXPECT(lr_bridge_reset(h) == LR_OK && result(h, t) == LR_OK && std::isnan(t[0]) && t[4] == 0, "reset");
    EXPECT(lr_bridge_accumulate(h, zeros, 100, 0, nullptr) == LR_OK && result(h, t) == LR_OK && t[4] == 100, "refilled to the brim, on the NULL stream");
    EXPECT(lr_bridge_accumulate(h, zeros, 1, 0, nullptr) == LR_ERR_INVALID && std::strstr(lr_last_error(), "exceed") != nullptr, "one too many");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    lr_bridge_destroy(h);
    lr_model_destroy(m);
}

static void solve_alone(void* stream) {
    std::vector<double> l1(5000, -3.0), l2(9000, -3.0);
    double t[LR_BRIDGE_ROWS];
    EXPECT(lr_bridge_solve(0, l1.data(), 5000, l2.data(), 9000, 0.0, 1e-10, 20, 0, t, stream) == LR_OK && t[4] == 5000 && t[5] == 9000, "solve from host memory");
    Dev d1(5000 * 8), d2(9000 * 8);
    EXPECT(lr_bridge_solve(0, (const double*)d1.p, 5000, (const double*)d2.p, 9000, 100.0, 1e-10, 20, 1, t, stream) == LR_OK && t[6] == 100, "solve from device memory");
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(lr_bridge_solve(0, l1.data(), 5000, l2.data(), 9000, 0.0, 1e-10, 20, 0, t, nullptr) == LR_OK, "solve");
    const long in_solve = hipstub_mallocs() - m0;
    EXPECT(in_solve == 3, "allocations of solve: %ld", in_solve);
    for (long k = 1; k <= in_solve; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = lr_bridge_solve(0, l1.data(), 5000, l2.data(), 9000, 0.0, 1e-10, 20, 0, t, nullptr); }
        EXPECT(rc == LR_ERR_NOMEM && hipstub_live_allocs() == live0, "allocation %ld of solve fails: rc %d, %ld leaked", k, rc, hipstub_live_allocs() - live0);
    }
}

static void failing_allocations(const Shape& s, const void* zeros) {
    lr_model* m = model(s.dtype, s.p, s.n);
    lr_bridge* h = nullptr;
    double t[LR_BRIDGE_ROWS];
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(create(m, s.p, 3000, 10, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_bridge_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
    const long in_feed = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_bridge_accumulate(h, zeros, 2000, 0, nullptr) == LR_OK, "a longer feed");
    const long in_regrow = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(result(h, t) == LR_OK && t[4] == 2003, "result");
    EXPECT(hipstub_mallocs() == m0, "result allocates nothing: its workspaces are create's");
    lr_bridge_destroy(h);
    h = nullptr;
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the accumulator", hipstub_live_allocs() - live0);
    EXPECT(in_create >= 6 && in_feed >= 1 && in_regrow >= 1, "allocations %ld / %ld / %ld", in_create, in_feed, in_regrow);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = create(m, s.p, 3000, 10, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h, "allocation %ld of %ld of create fails: rc %d", k, in_create, rc);
        if (h) lr_bridge_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "allocation %ld of create fails: %ld device buffers leaked", k, hipstub_live_allocs() - live0);
    }
    for (int regrow = 0; regrow < 2; ++regrow)
        for (long k = 1; k <= (regrow ? in_regrow : in_feed); ++k) {
            EXPECT(create(m, s.p, 3000, 10, &h) == LR_OK && h, "fresh");
            if (regrow) EXPECT(lr_bridge_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
            const double before = regrow ? 3 : 0;
            const long launches = hipstub_launches();
            int rc;
            { FailMallocAt failing(k); rc = lr_bridge_accumulate(h, zeros, 2000, 0, nullptr); }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == launches, "allocation %ld of accumulate fails (regrow %d) before anything is enqueued: rc %d", k, regrow, rc);
            int64_t n1 = -1;
            EXPECT(lr_bridge_terms(h, nullptr, nullptr, &n1, nullptr) == LR_OK && (double)n1 == before, "the count stays %g after a failed accumulate (%lld)", before, (long long)n1);
            EXPECT(lr_bridge_accumulate(h, zeros, 2000, 0, nullptr) == LR_OK && result(h, t) == LR_OK && t[4] == before + 2000, "usable after a failed accumulate");
            lr_bridge_destroy(h);
            h = nullptr;
            EXPECT(hipstub_live_allocs() == live0, "a failed accumulate leaked %ld device buffers", hipstub_live_allocs() - live0);
        }
    lr_model_destroy(m);
}

static void errors() {
    lr_model* m = model(LR_F32, 5);
    lr_bridge* h = nullptr;
    std::vector<double> mu(5, 0.0), cov = spd(5), t(LR_BRIDGE_ROWS, 0.0), l(8, -1.0);
    std::vector<float> draws((size_t)64 * 5, 0.f);
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    EXPECT(refused(lr_bridge_create(nullptr, mu.data(), cov.data(), 10, 10, 0, &h), "NULL") && refused(lr_bridge_create(m, nullptr, cov.data(), 10, 10, 0, &h), "NULL") &&
               refused(lr_bridge_create(m, mu.data(), nullptr, 10, 10, 0, &h), "NULL") && refused(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, nullptr), "NULL"),
           "NULL model / mu / cov / out");
    EXPECT(refused(lr_bridge_create(m, mu.data(), cov.data(), 0, 10, 0, &h), "positive") && refused(lr_bridge_create(m, mu.data(), cov.data(), 10, -1, 0, &h), "positive"), "counts");
    EXPECT(lr_bridge_create(m, mu.data(), cov.data(), LR_BRIDGE_MAX_DRAWS + 1, 10, 0, &h) == LR_ERR_UNSUPPORTED &&
               lr_bridge_create(m, mu.data(), cov.data(), 10, LR_BRIDGE_MAX_DRAWS + 1, 0, &h) == LR_ERR_UNSUPPORTED, "beyond the cap");
    for (double bad : {(double)INFINITY, (double)NAN}) {
        mu[2] = bad;
        EXPECT(refused(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, &h), "mu[2] is not finite"), "mu = %g", bad);
        mu[2] = 0.0;
        cov[3 * 5 + 1] = bad;
        EXPECT(refused(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, &h), "cov[3][1] is not finite"), "cov = %g", bad);
        cov[3 * 5 + 1] = 0.5;
    }
    cov[4 * 5 + 4] = 0.1;  // the last pivot goes negative
    EXPECT(refused(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, &h), "not positive definite: pivot 4"), "an indefinite matrix");
    cov[4 * 5 + 4] = 2.5;
    cov[0] = 0.0;
    EXPECT(refused(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, &h), "pivot 0"), "a zero variance");
    cov[0] = 2.5;
    EXPECT(h == nullptr, "no accumulator came out of a failed create");
    EXPECT(lr_bridge_create(m, mu.data(), cov.data(), 10, 10, 0, &h) == LR_OK && h, "create");
    EXPECT(refused(lr_bridge_accumulate(nullptr, draws.data(), 2, 0, nullptr), "NULL") && refused(lr_bridge_accumulate(h, nullptr, 2, 0, nullptr), "NULL") &&
               refused(lr_bridge_accumulate(h, draws.data(), 0, 0, nullptr), "positive") && refused(lr_bridge_accumulate(h, draws.data(), 11, 0, nullptr), "exceed"),
           "NULL accumulator / draws, S <= 0, too many");
    EXPECT(refused(lr_bridge_result(nullptr, 0, 1e-10, 10, t.data()), "NULL") && refused(lr_bridge_result(h, 0, 1e-10, 10, nullptr), "NULL") &&
               refused(lr_bridge_result(h, 0, -1.0, 10, t.data()), "tol") && refused(lr_bridge_result(h, 0, (double)NAN, 10, t.data()), "tol") &&
               refused(lr_bridge_result(h, 0, 1e-10, -1, t.data()), "maxit"), "result arguments");
    EXPECT(refused(lr_bridge_terms(nullptr, nullptr, nullptr, nullptr, nullptr), "NULL") && refused(lr_bridge_proposal(nullptr, nullptr, nullptr), "NULL") &&
               refused(lr_bridge_reset(nullptr), "NULL"), "NULL terms / proposal / reset");
    EXPECT(refused(lr_bridge_solve(0, nullptr, 8, l.data(), 8, 0, 1e-10, 10, 0, t.data(), nullptr), "NULL") && refused(lr_bridge_solve(0, l.data(), 0, l.data(), 8, 0, 1e-10, 10, 0, t.data(), nullptr), "positive") &&
               refused(lr_bridge_solve(0, l.data(), 8, l.data(), 8, 0, -1, 10, 0, t.data(), nullptr), "tol") &&
               lr_bridge_solve(0, l.data(), (int64_t)1 << 31, l.data(), 8, 0, 1e-10, 10, 0, t.data(), nullptr) == LR_ERR_UNSUPPORTED &&
               lr_bridge_solve(3, l.data(), 8, l.data(), 8, 0, 1e-10, 10, 0, t.data(), nullptr) == LR_ERR_HIP, "solve arguments");
    lr_bridge_destroy(h);
    lr_bridge_destroy(nullptr);
    lr_model_destroy(m);
}

int main() {
    const std::vector<unsigned char> zeros((size_t)3000 * 128 * 8, 0);  // zero-filled draws for everything below
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (int dtype : {LR_F32, LR_F64})
        for (const Shape& s : {Shape{dtype, 5, 50}, Shape{dtype, 8, 50}, Shape{dtype, 100, 20}, Shape{dtype, 3, 1300}, Shape{dtype, 1, 1}}) {
            life(s, zeros.data(), stream);
            failing_allocations(s, zeros.data());
        }
    solve_alone(stream);
    errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("bridge harness", "k_bridge_fill");
}
