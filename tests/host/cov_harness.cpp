// cov_harness.cpp -- TEST INFRASTRUCTURE: the host side of the covariance accumulator (include/logreg_hip_cov.h; lr_api.hip over
// csrc/lr_accum.h) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory
// is the host heap) and compiled with -fsanitize=address,undefined by tests/test_cov_cpu.py.  It drives the C ABI: both dtypes, a padded
// (5 -> 8, 100 -> 128) and an unpadded (8, 64) p, host and device input on a stream, each table of the result alone and all together,
// reset, host input one time step longer than a staging piece, every refused argument, and a failing device allocation at EVERY
// allocation of create, accumulate (first use and regrow) and result: LR_ERR_NOMEM, the count unchanged, nothing leaked, the handle
// usable afterwards.  With no-op kernels the tables hold the zeros the stub's allocator fills in: what is checked is the host logic
// (workspace sizes, the tile -> matrix map staying inside its buffers, every error path), not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"
#include "logreg_hip_cov.h"

struct Shape {
    int dtype;
    int64_t C;
    int p;
    size_t step() const { return (size_t)C * p * (dtype == LR_F32 ? 4 : 8); }
};

static int create(const Shape& s, lr_cov** h) {
    const std::vector<double> center((size_t)s.p, 0.5), scale((size_t)s.p, 2.0);
    return lr_cov_create(0, s.dtype, s.C, s.p, center.data(), scale.data(), h);
}

// every table alone, then all four: the first cell of each, the count
static int result(const Shape& s, lr_cov* h, int64_t* n, double* first) {
    const size_t pp = (size_t)s.p * s.p;
    std::vector<double> M(pp, 7.0), Q(pp, 7.0), sum((size_t)s.p, 7.0), S((size_t)s.C * s.p, 7.0);
    int rc = lr_cov_result(h, M.data(), nullptr, nullptr, nullptr, n);
    if (!rc) rc = lr_cov_result(h, nullptr, Q.data(), nullptr, nullptr, n);
    if (!rc) rc = lr_cov_result(h, nullptr, nullptr, sum.data(), nullptr, n);
    if (!rc) rc = lr_cov_result(h, nullptr, nullptr, nullptr, S.data(), n);
    if (!rc) rc = lr_cov_result(h, M.data(), Q.data(), sum.data(), S.data(), n);
    if (!rc) {
        bool untouched = false, same = true;
        for (size_t i = 0; i < pp; ++i) untouched = untouched || M[i] == 7.0 || Q[i] == 7.0;
        for (double v : sum) untouched = untouched || v == 7.0;
        for (double v : S) untouched = untouched || v == 7.0;
        for (int i = 0; i < s.p; ++i)
            for (int j = 0; j < s.p; ++j) same = same && std::memcmp(&M[(size_t)i * s.p + j], &M[(size_t)j * s.p + i], 8) == 0;
        EXPECT(!untouched && same, "result: every entry of every table is written, moment is symmetric (C %lld, p %d)", (long long)s.C, s.p);
    }
    first[0] = M[0];
    first[1] = Q[pp - 1];
    first[2] = sum[s.p - 1];
    first[3] = S[(size_t)s.C * s.p - 1];
    return rc;
}
static bool all_nan(const double* f) { return std::isnan(f[0]) && std::isnan(f[1]) && std::isnan(f[2]) && std::isnan(f[3]); }

static void life(const Shape& s, const void* zeros, void* stream) {
    lr_cov* h = nullptr;
    int64_t n = -1;
    double f[4];
    EXPECT(create(s, &h) == LR_OK && h, "create (C %lld, p %d)", (long long)s.C, s.p);
    if (!h) return;
    EXPECT(result(s, h, &n, f) == LR_OK && n == 0 && all_nan(f), "NaN before the first draw (n %lld)", (long long)n);
    Dev dev(7 * s.step());
    EXPECT(dev.p != nullptr, "device input");
    const long l0 = hipstub_launches_on(stream), k0 = hipstub_launches_of("k_cov_accumulate");
    EXPECT(lr_cov_accumulate(h, zeros, 5, 0, stream) == LR_OK, "host input");
    EXPECT(lr_cov_accumulate(h, dev.p, 7, 1, stream) == LR_OK, "device input");
    EXPECT(hipstub_launches_of("k_cov_accumulate") == k0 + 2 && hipstub_launches_on(stream) >= l0 + 2, "one piece each, on the caller's stream");
    EXPECT(result(s, h, &n, f) == LR_OK && n == 12 && !all_nan(f), "result of 12 (n %lld)", (long long)n);
    EXPECT(lr_cov_result(h, nullptr, nullptr, nullptr, nullptr, &n) == LR_OK && n == 12 && lr_cov_result(h, nullptr, nullptr, nullptr, nullptr, nullptr) == LR_OK, "the count alone");
    EXPECT(lr_cov_reset(h) == LR_OK && result(s, h, &n, f) == LR_OK && n == 0 && all_nan(f), "reset");
    EXPECT(lr_cov_accumulate(h, zeros, 3, 0, nullptr) == LR_OK && result(s, h, &n, f) == LR_OK && n == 3, "more draws after a reset, on the NULL stream");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    lr_cov_destroy(h);
}

static void two_pieces(const Shape& s, int64_t piece, const void* zeros, void* stream) {
    lr_cov* h = nullptr;
    int64_t n = -1;
    EXPECT(create(s, &h) == LR_OK && h, "create");
    if (!h) return;
    const long k0 = hipstub_launches_of("k_cov_accumulate");
    EXPECT(lr_cov_accumulate(h, zeros, piece, 0, stream) == LR_OK && hipstub_launches_of("k_cov_accumulate") == k0 + 1, "%lld steps are one piece", (long long)piece);
    EXPECT(lr_cov_accumulate(h, zeros, 1, 0, stream) == LR_OK && hipstub_launches_of("k_cov_accumulate") == k0 + 2, "one more");
    EXPECT(lr_cov_reset(h) == LR_OK, "reset");
    EXPECT(lr_cov_accumulate(h, zeros, piece + 1, 0, stream) == LR_OK && hipstub_launches_of("k_cov_accumulate") == k0 + 4, "%lld steps are two pieces", (long long)piece + 1);
    EXPECT(lr_cov_result(h, nullptr, nullptr, nullptr, nullptr, &n) == LR_OK && n == piece + 1, "all of them counted (n %lld)", (long long)n);
    lr_cov_destroy(h);
}

static void failing_allocations(const Shape& s, const void* zeros) {
    lr_cov* h = nullptr;
    int64_t n = -1;
    double f[4];
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(create(s, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_cov_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
    const long in_feed = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_cov_accumulate(h, zeros, 40, 0, nullptr) == LR_OK, "a longer feed");
    const long in_regrow = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(result(s, h, &n, f) == LR_OK && n == 43, "result");
    const long in_result = hipstub_mallocs() - m0;
    lr_cov_destroy(h);
    h = nullptr;
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the accumulator", hipstub_live_allocs() - live0);
    EXPECT(in_create >= 1 && in_feed >= 1 && in_regrow >= 1 && in_regrow <= in_feed && in_result >= 1, "allocations %ld / %ld / %ld / %ld", in_create, in_feed, in_regrow, in_result);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = create(s, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h, "allocation %ld of %ld of create fails: rc %d", k, in_create, rc);
        if (h) lr_cov_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "allocation %ld of create fails: %ld device buffers leaked", k, hipstub_live_allocs() - live0);
    }
    for (int regrow = 0; regrow < 2; ++regrow)
        for (long k = 1; k <= (regrow ? in_regrow : in_feed); ++k) {
            EXPECT(create(s, &h) == LR_OK && h, "fresh");
            if (regrow) EXPECT(lr_cov_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
            const int64_t before = regrow ? 3 : 0;
            int rc;
            { FailMallocAt failing(k); rc = lr_cov_accumulate(h, zeros, 40, 0, nullptr); }
            EXPECT(rc == LR_ERR_NOMEM, "allocation %ld of accumulate fails (regrow %d): rc %d", k, regrow, rc);
            EXPECT(result(s, h, &n, f) == LR_OK && n == before, "the count stays %lld after a failed accumulate (n %lld)", (long long)before, (long long)n);
            EXPECT(lr_cov_accumulate(h, zeros, 40, 0, nullptr) == LR_OK && result(s, h, &n, f) == LR_OK && n == before + 40, "usable after a failed accumulate");
            lr_cov_destroy(h);
            h = nullptr;
            EXPECT(hipstub_live_allocs() == live0, "a failed accumulate leaked %ld device buffers", hipstub_live_allocs() - live0);
        }
    for (long k = 1; k <= in_result; ++k) {
        EXPECT(create(s, &h) == LR_OK && h && lr_cov_accumulate(h, zeros, 43, 0, nullptr) == LR_OK, "fresh");
        n = -1;
        int rc;
        { FailMallocAt failing(k); rc = result(s, h, &n, f); }  // (the k-th allocation of the whole sequence of result calls)
        EXPECT(rc == LR_ERR_NOMEM && n == 43, "allocation %ld of %ld of result fails: rc %d, n %lld", k, in_result, rc, (long long)n);
        EXPECT(result(s, h, &n, f) == LR_OK && n == 43 && lr_cov_accumulate(h, zeros, 2, 0, nullptr) == LR_OK, "usable after a failed result");
        lr_cov_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "a failed result leaked %ld device buffers", hipstub_live_allocs() - live0);
    }
}

static void errors() {
    std::vector<double> center(5, 0.0), scale(5, 1.0), t(4096, 0.0);
    std::vector<float> draws((size_t)64 * 8 * 5, 0.f);
    int64_t n = 0;
    lr_cov* h = nullptr;
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    EXPECT(refused(lr_cov_create(0, LR_F32, 8, 5, center.data(), scale.data(), nullptr), "NULL") && refused(lr_cov_create(0, LR_F32, 8, 5, nullptr, scale.data(), &h), "NULL") &&
               refused(lr_cov_create(0, LR_F32, 8, 5, center.data(), nullptr, &h), "NULL"), "NULL out / center / scale");
    EXPECT(refused(lr_cov_create(0, LR_F32, 0, 5, center.data(), scale.data(), &h), "positive") && refused(lr_cov_create(0, LR_F32, -3, 5, center.data(), scale.data(), &h), "positive") &&
               refused(lr_cov_create(0, LR_F32, 8, 0, center.data(), scale.data(), &h), "positive") && refused(lr_cov_create(0, LR_F32, 8, -1, center.data(), scale.data(), &h), "positive"), "C, p");
    {
        const std::vector<double> c129(129, 0.0), s129(129, 1.0);
        EXPECT(refused(lr_cov_create(0, LR_F32, 8, LR_COV_MAX_P + 1, c129.data(), s129.data(), &h), "1..128"), "p beyond the widest kernel");
    }
    EXPECT(refused(lr_cov_create(0, 7, 8, 5, center.data(), scale.data(), &h), "dtype"), "dtype");
    for (double bad : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
        scale[3] = bad;
        EXPECT(refused(lr_cov_create(0, LR_F32, 8, 5, center.data(), scale.data(), &h), "scale > 0"), "scale = %g", bad);
    }
    scale[3] = 1.0;
    for (double bad : {(double)INFINITY, -(double)INFINITY, (double)NAN}) {
        center[0] = bad;
        EXPECT(refused(lr_cov_create(0, LR_F32, 8, 5, center.data(), scale.data(), &h), "finite center"), "center = %g", bad);
    }
    center[0] = 0.0;
    EXPECT(lr_cov_create(0, LR_F32, (int64_t)1 << 40, 5, center.data(), scale.data(), &h) == LR_ERR_UNSUPPORTED, "chains beyond the grid");
    EXPECT(lr_cov_create(5, LR_F32, 8, 5, center.data(), scale.data(), &h) == LR_ERR_HIP && h == nullptr, "device ordinal");
    EXPECT(h == nullptr, "no accumulator came out of a failed create");
    EXPECT(lr_cov_create(0, LR_F32, 8, 5, center.data(), scale.data(), &h) == LR_OK && h, "create");
    EXPECT(refused(lr_cov_accumulate(nullptr, draws.data(), 2, 0, nullptr), "NULL") && refused(lr_cov_accumulate(h, nullptr, 2, 0, nullptr), "NULL") &&
               refused(lr_cov_accumulate(h, draws.data(), 0, 0, nullptr), "positive") && refused(lr_cov_accumulate(h, draws.data(), -1, 0, nullptr), "positive"),
           "NULL accumulator / block, k <= 0");
    EXPECT(refused(lr_cov_result(nullptr, t.data(), nullptr, nullptr, nullptr, &n), "NULL") && refused(lr_cov_reset(nullptr), "NULL"), "NULL result / reset");
    EXPECT(lr_cov_result(h, nullptr, nullptr, nullptr, nullptr, &n) == LR_OK && n == 0, "refused calls left it empty");
    lr_cov_destroy(h);
    lr_cov_destroy(nullptr);
    hipstub_set_devices(0);
    h = nullptr;
    EXPECT(lr_cov_create(0, LR_F32, 8, 5, center.data(), scale.data(), &h) == LR_ERR_HIP && h == nullptr && std::strstr(lr_last_error(), "hipGetDeviceCount") != nullptr, "without a device");
    hipstub_set_devices(1);
}

int main() {
    // zero-filled input for everything below: 65 time steps of the 8192 x 64 float64 block (64 steps of it are one 256 MB staging piece)
    const int64_t bigC = 8192;
    const int bigp = 64;
    const std::vector<unsigned char> zeros((size_t)65 * bigC * bigp * 8, 0);
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (int dtype : {LR_F32, LR_F64})
        for (const Shape& s : {Shape{dtype, 37, 5}, Shape{dtype, 37, 8}, Shape{dtype, 3, 100}, Shape{dtype, 600, 64}, Shape{dtype, 1, 1}, Shape{dtype, 9000, 3}}) {
            life(s, zeros.data(), stream);
            failing_allocations(s, zeros.data());
        }
    two_pieces(Shape{LR_F64, bigC, bigp}, 64, zeros.data(), stream);
    errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("cov harness", "k_cov_accumulate");
}
