// rank_harness.cpp -- TEST INFRASTRUCTURE: the host side of the rank-diagnostics accumulator (include/logreg_hip_rank.h; lr_api.hip over
// csrc/lr_accum.h) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory
// is the host heap) and built under the sanitizers by tests/host_build.py.  It drives the C ABI: both dtypes, one and several
// coordinates, fewer draws than one sort tile and more (global merge launches), host and device input on a stream, result, ranks,
// reset, every refused argument, and a failing device allocation at EVERY allocation of create, accumulate, result and ranks:
// LR_ERR_NOMEM, the count unchanged, nothing enqueued, nothing leaked, the handle usable afterwards.  With no-op kernels the tables hold
// the zeros the stub's allocator fills in (W = 0: NaN): what is checked is the host logic (workspace sizes, the launch sequence, every
// error path), not arithmetic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"
#include "logreg_hip_rank.h"

struct Shape {
    int dtype, p;
    int64_t C, steps;
    size_t row() const { return (size_t)C * p * (dtype == LR_F32 ? 4 : 8); }
};

static int result(lr_rank* h, int p, std::vector<double>& t, int64_t* n) {
    t.assign((size_t)LR_RANK_ROWS * p, 7.0);
    return lr_rank_result(h, t.data(), n);
}

static bool all_nan_but_counts(const std::vector<double>& t, int p) {
    for (int r = 0; r < LR_RANK_ROWS; ++r)
        for (int j = 0; j < p; ++j)
            if (r == 11 ? t[(size_t)r * p + j] != 0.0 : r >= 8 && r <= 10 ? false : !std::isnan(t[(size_t)r * p + j])) return false;
    return true;
}

static long merges_wanted(int64_t S) {  // global compare-exchange launches of one sort of S keys
    int64_t N = 2;
    while (N < S) N <<= 1;
    long g = 0;
    for (int64_t k = 2 * 8192; k <= N; k <<= 1)
        for (int64_t j = k >> 1; j >= 8192; j >>= 1) ++g;
    return g;
}

static void life(const Shape& s, const void* zeros, void* stream) {
    lr_rank* h = nullptr;
    std::vector<double> t;
    int64_t n = -1;
    EXPECT(lr_rank_create(0, s.dtype, s.C, s.p, s.steps, 63, &h) == LR_OK && h, "create (C %lld, p %d, steps %lld)", (long long)s.C, s.p, (long long)s.steps);
    if (!h) return;
    const long l00 = hipstub_launches();
    EXPECT(result(h, s.p, t, &n) == LR_OK && n == 0 && std::isnan(t[0]) && t[(size_t)11 * s.p] == 0.0 && hipstub_launches() == l00, "NaN before the first draw, nothing launched");
    const int64_t a = s.steps / 2, b = s.steps - a;
    Dev dev((size_t)b * s.row());
    EXPECT(dev.p != nullptr, "device input");
    EXPECT(lr_rank_accumulate(h, zeros, a, 0, stream) == LR_OK, "host input");
    EXPECT(lr_rank_accumulate(h, dev.p, b, 1, stream) == LR_OK, "device input");
    EXPECT(lr_rank_accumulate(h, zeros, 1, 0, stream) == LR_ERR_INVALID && std::strstr(lr_last_error(), "exceed") != nullptr, "one too many");
    const long s0 = hipstub_launches_of("k_rank_sort_tile"), g0 = hipstub_launches_of("k_rank_merge_global"), z0 = hipstub_launches_of("k_rank_lookup"), t0 = hipstub_launches_of("k_rank_transform"),
               lag0 = hipstub_launches_of("k_rank_lag"), on0 = hipstub_launches_on(stream);
    EXPECT(result(h, s.p, t, &n) == LR_OK && n == s.steps, "result (n %lld)", (long long)n);
    const int64_t S = s.steps / 2 * 2 * s.C;
    const long g = merges_wanted(S);
    if (s.steps >= 4) {
        EXPECT(all_nan_but_counts(t, s.p), "zero tables give NaN, never a finite number");
        EXPECT(hipstub_launches_of("k_rank_merge_global") == g0 + 2 * g && hipstub_launches_of("k_rank_lookup") == z0 + 2 && hipstub_launches_of("k_rank_transform") == t0 + 2 && hipstub_launches_of("k_rank_lag") == lag0 + 1,
               "two sorts of %ld global merges, two lookups and two transforms, one lag launch (one batch of coordinates)", g);
        EXPECT(hipstub_launches_of("k_rank_sort_tile") > s0 && hipstub_launches_on(stream) > on0, "on the caller's stream");
    } else {
        EXPECT(std::isnan(t[0]) && hipstub_launches_of("k_rank_sort_tile") == s0, "n < 4: NaN, nothing sorted");
    }
    std::vector<int64_t> r2((size_t)S, -5);
    std::vector<double> z((size_t)S, 7.0);
    int64_t used = -1;
    EXPECT(lr_rank_ranks(h, s.p - 1, 0, r2.data(), z.data(), &used) == LR_OK && used == s.steps / 2 * 2, "ranks (used %lld)", (long long)used);
    EXPECT(lr_rank_ranks(h, 0, 1, r2.data(), nullptr, nullptr) == LR_OK, "folded ranks without z");
    EXPECT(lr_rank_reset(h) == LR_OK && result(h, s.p, t, &n) == LR_OK && n == 0 && std::isnan(t[0]), "reset");
    EXPECT(lr_rank_accumulate(h, zeros, s.steps, 0, nullptr) == LR_OK && result(h, s.p, t, &n) == LR_OK && n == s.steps, "refilled to the brim, on the NULL stream");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    lr_rank_destroy(h);
}

static void failing_allocations(const Shape& s, const void* zeros) {
    lr_rank* h = nullptr;
    std::vector<double> t;
    std::vector<int64_t> r2((size_t)s.steps * s.C);
    int64_t n = -1;
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(lr_rank_create(0, s.dtype, s.C, s.p, s.steps, 7, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_rank_accumulate(h, zeros, s.steps - 1, 0, nullptr) == LR_OK, "feed");
    const long in_feed = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(result(h, s.p, t, &n) == LR_OK && n == s.steps - 1, "result");
    const long in_result = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(result(h, s.p, t, &n) == LR_OK, "result again");
    EXPECT(hipstub_mallocs() == m0, "a second result allocates nothing");
    lr_rank_destroy(h);
    h = nullptr;
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the accumulator", hipstub_live_allocs() - live0);
    EXPECT(in_create == 1 && in_feed == 1 && in_result == 1, "allocations %ld / %ld / %ld", in_create, in_feed, in_result);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = lr_rank_create(0, s.dtype, s.C, s.p, s.steps, 7, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h && hipstub_live_allocs() == live0, "allocation %ld of create fails: rc %d, %ld leaked", k, rc, hipstub_live_allocs() - live0);
        if (h) lr_rank_destroy(h);
        h = nullptr;
    }
    EXPECT(lr_rank_create(0, s.dtype, s.C, s.p, s.steps, 7, &h) == LR_OK && h, "fresh");
    for (long k = 1; k <= in_feed; ++k) {
        const long launches = hipstub_launches();
        int rc;
        { FailMallocAt failing(k); rc = lr_rank_accumulate(h, zeros, s.steps - 1, 0, nullptr); }
        EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == launches, "allocation %ld of accumulate fails before anything is enqueued: rc %d", k, rc);
        EXPECT(result(h, s.p, t, &n) == LR_OK && n == 0, "the count stays 0 after a failed accumulate (%lld)", (long long)n);
    }
    EXPECT(lr_rank_accumulate(h, zeros, s.steps - 1, 0, nullptr) == LR_OK, "usable after a failed accumulate");
    for (long k = 1; k <= in_result; ++k) {
        const long launches = hipstub_launches();
        int rc;
        { FailMallocAt failing(k); rc = result(h, s.p, t, &n); }
        EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == launches, "allocation %ld of result fails before anything is enqueued: rc %d", k, rc);
        { FailMallocAt failing(k); rc = lr_rank_ranks(h, 0, 1, r2.data(), nullptr, &n); }
        EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == launches, "allocation %ld of ranks fails before anything is enqueued: rc %d", k, rc);
    }
    EXPECT(result(h, s.p, t, &n) == LR_OK && n == s.steps - 1, "usable after a failed result: the draws are still there (%lld)", (long long)n);
    EXPECT(lr_rank_ranks(h, 0, 0, r2.data(), nullptr, &n) == LR_OK && n == (s.steps - 1) / 2 * 2, "ranks after it");
    EXPECT(lr_rank_accumulate(h, zeros, 1, 0, nullptr) == LR_OK && result(h, s.p, t, &n) == LR_OK && n == s.steps, "and more draws may follow");
    lr_rank_destroy(h);
    EXPECT(hipstub_live_allocs() == live0, "failed calls leaked %ld device buffers", hipstub_live_allocs() - live0);
}

static void errors() {
    lr_rank* h = nullptr;
    std::vector<double> t((size_t)LR_RANK_ROWS * 3), x((size_t)8 * 5 * 3, 0.0);
    std::vector<int64_t> r2(40);
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    EXPECT(refused(lr_rank_create(0, LR_F64, 5, 3, 8, 63, nullptr), "NULL"), "NULL out");
    EXPECT(refused(lr_rank_create(0, LR_F64, 0, 3, 8, 63, &h), "positive") && refused(lr_rank_create(0, LR_F64, 5, 0, 8, 63, &h), "positive") &&
               refused(lr_rank_create(0, LR_F64, 5, 3, 0, 63, &h), "positive"), "C, p, max_steps");
    EXPECT(refused(lr_rank_create(0, LR_F64, 5, 3, 8, 64, &h), "odd") && refused(lr_rank_create(0, LR_F64, 5, 3, 8, 257, &h), "odd") &&
               refused(lr_rank_create(0, LR_F64, 5, 3, 8, 0, &h), "odd"), "max_lag");
    EXPECT(refused(lr_rank_create(0, 7, 5, 3, 8, 63, &h), "dtype"), "dtype");
    EXPECT(lr_rank_create(0, LR_F32, 4097, 3, 4096, 63, &h) == LR_ERR_UNSUPPORTED && std::strstr(lr_last_error(), "LR_RANK_MAX_DRAWS") != nullptr &&
               lr_rank_create(0, LR_F32, LR_RANK_MAX_DRAWS + 1, 3, 1, 63, &h) == LR_ERR_UNSUPPORTED &&
               lr_rank_create(0, LR_F32, 3, 3, INT64_MAX, 63, &h) == LR_ERR_UNSUPPORTED, "beyond the cap");
    EXPECT(lr_rank_create(3, LR_F32, 5, 3, 8, 63, &h) == LR_ERR_HIP, "a device that is not there");
    EXPECT(h == nullptr, "no accumulator came out of a failed create");
    EXPECT(lr_rank_create(0, LR_F64, 5, 3, 8, 63, &h) == LR_OK && h, "create");
    EXPECT(refused(lr_rank_accumulate(nullptr, x.data(), 2, 0, nullptr), "NULL") && refused(lr_rank_accumulate(h, nullptr, 2, 0, nullptr), "NULL") &&
               refused(lr_rank_accumulate(h, x.data(), 0, 0, nullptr), "positive") && refused(lr_rank_accumulate(h, x.data(), 9, 0, nullptr), "exceed"),
           "NULL accumulator / block, k <= 0, too many");
    EXPECT(refused(lr_rank_result(nullptr, t.data(), nullptr), "NULL") && refused(lr_rank_result(h, nullptr, nullptr), "NULL"), "result arguments");
    EXPECT(refused(lr_rank_ranks(nullptr, 0, 0, r2.data(), nullptr, nullptr), "NULL") && refused(lr_rank_ranks(h, 0, 0, nullptr, nullptr, nullptr), "NULL") &&
               refused(lr_rank_ranks(h, 3, 0, r2.data(), nullptr, nullptr), "coordinate") && refused(lr_rank_ranks(h, -1, 0, r2.data(), nullptr, nullptr), "coordinate"),
           "ranks arguments");
    EXPECT(refused(lr_rank_reset(nullptr), "NULL"), "NULL reset");
    int64_t n = -1;
    EXPECT(lr_rank_result(h, t.data(), &n) == LR_OK && n == 0, "refused calls left it empty");
    EXPECT(lr_rank_accumulate(h, x.data(), 8, 0, nullptr) == LR_OK && lr_rank_result(h, t.data(), &n) == LR_OK && n == 8, "filled");
    lr_rank_destroy(h);
    lr_rank_destroy(nullptr);
}

int main() {
    const std::vector<unsigned char> zeros((size_t)40 * 600 * 3 * 8, 0);  // zero-filled draws for everything below
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (int dtype : {LR_F32, LR_F64})
        for (const Shape& s : {Shape{dtype, 1, 3, 9}, Shape{dtype, 3, 5, 64}, Shape{dtype, 2, 67, 130}, Shape{dtype, 3, 600, 40}, Shape{dtype, 2, 4, 3}}) {
            life(s, zeros.data(), stream);
            if (s.steps >= 5) failing_allocations(s, zeros.data());  // (a result of fewer than 4 steps allocates nothing)
        }
    errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("rank harness", "k_rank_sort_tile");
}
