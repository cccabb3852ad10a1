// ppc_harness.cpp -- TEST INFRASTRUCTURE: the host side of the predictive-check accumulator (include/logreg_hip_ppc.h; lr_api.hip over
// csrc/lr_accum.h) as a program of its own, linked against tests/host/hip_stub.cpp (kernel launches are validated no-ops, device memory
// is the host heap) and built under the sanitizers by tests/host_build.py.  It drives the C ABI: both dtypes, a padded (5 -> 8, 100 -> 128)
// and an unpadded (8) p, one row and more rows than a tile, with and without labels and groups, host and device input on a stream, terms,
// result, reset; every refused argument, with no device allocation and no launch behind it; a failing device allocation at EVERY
// allocation of create, accumulate (first use and regrow) and terms: LR_ERR_NOMEM, the count unchanged, nothing leaked, the handle usable
// afterwards; and the sub-batch rule: the launches of a long feed at a million rows, cut at multiples of 4 of the draw index, with a
// workspace that does not grow with S.  With no-op kernels the tables hold the zeros the stub's allocator fills in: what is checked is
// the host logic, not arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness.h"
#include "logreg_hip_ppc.h"

struct Shape {
    int dtype, p;
    int64_t n;
    int G;
    size_t draw() const { return (size_t)p * (dtype == LR_F32 ? 4 : 8); }
};

static std::vector<int32_t> labels(int64_t n, int G) {
    std::vector<int32_t> g((size_t)n);
    for (int64_t i = 0; i < n; ++i) g[(size_t)i] = (int32_t)(i % G);
    return g;
}

static int create(lr_model* m, const Shape& s, lr_ppc** h) {
    const std::vector<int32_t> g = labels(s.n, s.G);
    return lr_ppc_create(m, nullptr, nullptr, s.n, s.G > 1 ? g.data() : nullptr, s.G, 7, h);
}

static int64_t count(lr_ppc* h) {
    int64_t n = -1;
    return lr_ppc_result(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n) == LR_OK ? n : -2;
}

static void life(const Shape& s, const void* zeros, void* stream) {
    lr_model* m = model(s.dtype, s.p, s.n);
    lr_ppc* h = nullptr;
    EXPECT(create(m, s, &h) == LR_OK && h, "create (p %d, n %lld, G %d)", s.p, (long long)s.n, s.G);
    if (!h) return;
    std::vector<uint64_t> hist((size_t)(s.n + s.G), 7), ones((size_t)s.n, 7);
    uint64_t counts[2] = {7, 7};
    double mom[LR_PPC_MOMENTS] = {7, 7, 7, 7};
    std::vector<int64_t> t_obs((size_t)s.G, -7), n_g((size_t)s.G, -7);
    int64_t n = -1, rows = 0, obs = 0;
    EXPECT(lr_ppc_result(h, hist.data(), ones.data(), counts, mom, t_obs.data(), n_g.data(), &n) == LR_OK && n == 0 && counts[0] == 0 && counts[1] == 0 &&
               std::isnan(mom[0]) && std::isnan(mom[3]) && hist[0] == 0 && ones[(size_t)s.n - 1] == 0, "empty before the first draw");
    for (int g = 0; g < s.G; ++g) {
        rows += n_g[(size_t)g];
        obs += t_obs[(size_t)g];
    }
    EXPECT(rows == s.n && obs == s.n / 2, "group sizes add up to %lld rows (%lld), observed ones %lld", (long long)s.n, (long long)rows, (long long)obs);
    Dev dev(7 * s.draw());
    EXPECT(dev.p != nullptr, "device input");
    const long p0 = hipstub_launches_of("k_ppc_partial"), f0 = hipstub_launches_of("k_ppc_fold"), m0 = hipstub_launches_of("k_ppc_moments"), l0 = hipstub_launches_on(stream);
    EXPECT(lr_ppc_accumulate(h, zeros, 5, 0, stream) == LR_OK && count(h) == 5, "host input");
    EXPECT(lr_ppc_accumulate(h, dev.p, 7, 1, stream) == LR_OK && count(h) == 12, "device input");
    EXPECT(hipstub_launches_of("k_ppc_partial") == p0 + 2 && hipstub_launches_of("k_ppc_fold") == f0 + 2 && hipstub_launches_of("k_ppc_moments") == m0 + 2 &&
               hipstub_launches_on(stream) >= l0 + 8, "one sub-batch each, on the caller's stream");
    std::vector<int32_t> c((size_t)9 * s.G, 7);
    std::vector<double> d(18, 7.0);
    std::vector<uint32_t> bits((size_t)9 * ((s.n + 31) / 32), 7);
    EXPECT(lr_ppc_terms(h, zeros, 9, 3, 0, stream, c.data(), d.data(), bits.data()) == LR_OK && c.back() != 7 && d.back() != 7.0 && bits.back() != 7, "terms");
    EXPECT(lr_ppc_terms(h, dev.p, 7, 0, 1, stream, c.data(), d.data(), nullptr) == LR_OK, "terms of device input without the bits");
    EXPECT(count(h) == 12 && hipstub_launches_of("k_ppc_moments") == m0 + 2, "terms accumulate nothing");
    EXPECT(lr_ppc_reset(h) == LR_OK && count(h) == 0, "reset");
    EXPECT(lr_ppc_accumulate(h, zeros, 100, 0, nullptr) == LR_OK && count(h) == 100, "refilled on the NULL stream");
    EXPECT(lr_stream_sync(0, stream) == LR_OK, "sync");
    lr_ppc_destroy(h);
    // rows and labels of its own, with and without labels
    Design keep;
    lr_model* m2 = model(s.dtype, s.p, s.n, 1.0, false, &keep);
    for (int with_y = 0; with_y < 2; ++with_y) {
        h = nullptr;
        EXPECT(lr_ppc_create(m2, keep.X.data(), with_y ? keep.y.data() : nullptr, s.n, nullptr, 1, 0, &h) == LR_OK && h, "create on X_new (labels %d)", with_y);
        if (!h) continue;
        EXPECT(lr_ppc_result(h, nullptr, nullptr, nullptr, nullptr, t_obs.data(), n_g.data(), nullptr) == LR_OK && n_g[0] == s.n && t_obs[0] == (with_y ? s.n / 2 : -1),
               "observed count with labels %d: %lld", with_y, (long long)t_obs[0]);
        EXPECT(lr_ppc_accumulate(h, zeros, 3, 0, nullptr) == LR_OK && count(h) == 3, "feed");
        lr_ppc_destroy(h);
    }
    lr_model_destroy(m2);
    lr_model_destroy(m);
}

static void failing_allocations(const Shape& s, const void* zeros) {
    lr_model* m = model(s.dtype, s.p, s.n);
    lr_ppc* h = nullptr;
    const long live0 = hipstub_live_allocs();
    long m0 = hipstub_mallocs();
    EXPECT(create(m, s, &h) == LR_OK && h, "create");
    const long in_create = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_ppc_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
    const long in_feed = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(lr_ppc_accumulate(h, zeros, 2000, 0, nullptr) == LR_OK, "a longer feed");
    const long in_regrow = hipstub_mallocs() - m0;
    m0 = hipstub_mallocs();
    EXPECT(count(h) == 2003 && hipstub_mallocs() == m0, "result allocates nothing");
    std::vector<int32_t> c((size_t)2500 * s.G);
    std::vector<double> d(5000);
    std::vector<uint32_t> bits((size_t)2500 * ((s.n + 31) / 32));
    EXPECT(lr_ppc_terms(h, zeros, 2500, 0, 0, nullptr, c.data(), d.data(), bits.data()) == LR_OK, "terms");
    const long in_terms = hipstub_mallocs() - m0;
    lr_ppc_destroy(h);
    h = nullptr;
    EXPECT(hipstub_live_allocs() == live0, "%ld device buffers outlive the accumulator", hipstub_live_allocs() - live0);
    EXPECT(in_create >= 4 && in_feed >= 4 && in_regrow >= 4 && in_terms >= 1, "allocations %ld / %ld / %ld / %ld", in_create, in_feed, in_regrow, in_terms);
    for (long k = 1; k <= in_create; ++k) {
        int rc;
        { FailMallocAt failing(k); rc = create(m, s, &h); }
        EXPECT(rc == LR_ERR_NOMEM && !h, "allocation %ld of %ld of create fails: rc %d", k, in_create, rc);
        if (h) lr_ppc_destroy(h);
        h = nullptr;
        EXPECT(hipstub_live_allocs() == live0, "allocation %ld of create fails: %ld device buffers leaked", k, hipstub_live_allocs() - live0);
    }
    for (int what = 0; what < 3; ++what) {  // first feed, regrow, terms
        const long most = what == 0 ? in_feed : what == 1 ? in_regrow : in_terms;
        for (long k = 1; k <= most; ++k) {
            EXPECT(create(m, s, &h) == LR_OK && h, "fresh");
            if (what) EXPECT(lr_ppc_accumulate(h, zeros, 3, 0, nullptr) == LR_OK, "feed");
            if (what == 2) EXPECT(lr_ppc_accumulate(h, zeros, 2000, 0, nullptr) == LR_OK, "a longer feed");
            const int64_t before = count(h);
            const long launches = hipstub_launches();
            int rc;
            {
                FailMallocAt failing(k);
                rc = what == 2 ? lr_ppc_terms(h, zeros, 2500, 0, 0, nullptr, c.data(), d.data(), bits.data()) : lr_ppc_accumulate(h, zeros, 2000, 0, nullptr);
            }
            EXPECT(rc == LR_ERR_NOMEM && hipstub_launches() == launches, "allocation %ld fails (case %d) before anything is enqueued: rc %d", k, what, rc);
            EXPECT(count(h) == before, "the count stays %lld after a failed call (%lld)", (long long)before, (long long)count(h));
            EXPECT(lr_ppc_accumulate(h, zeros, 2000, 0, nullptr) == LR_OK && count(h) == before + 2000, "usable after a failed call");
            lr_ppc_destroy(h);
            h = nullptr;
            EXPECT(hipstub_live_allocs() == live0, "a failed call leaked %ld device buffers", hipstub_live_allocs() - live0);
        }
    }
    lr_model_destroy(m);
}

// A million rows: 3907 tiles, 16 + 4 G bytes per (tile, draw), 64 MB of partials: 856 draws per sub-batch at G = 1 and 116 at G = 32.
static void sub_batches() {
    for (const Shape& s : {Shape{LR_F32, 4, 1000000, 1}, Shape{LR_F64, 4, 1000000, 32}}) {  // (p = 4 is a kernel width: no padded copy, whose size follows S)
        const int64_t sub = s.G == 1 ? 856 : 116;
        lr_model* m = model(s.dtype, s.p, s.n);
        lr_ppc* h = nullptr;
        EXPECT(create(m, s, &h) == LR_OK && h, "create at a million rows");
        if (!h) continue;
        Dev dev(3000 * s.draw());
        long p0 = hipstub_launches_of("k_ppc_partial");
        EXPECT(lr_ppc_accumulate(h, dev.p, 1, 1, nullptr) == LR_OK, "one draw: the next call starts at s = 1");
        EXPECT(hipstub_launches_of("k_ppc_partial") == p0 + 1, "one launch");
        p0 = hipstub_launches_of("k_ppc_partial");
        const int64_t S = 2 * sub + 50;  // [1, sub) [sub, 2 sub) [2 sub, 2 sub + 51): the cuts at multiples of 4 of the draw index
        EXPECT(lr_ppc_accumulate(h, dev.p, S, 1, nullptr) == LR_OK && count(h) == S + 1, "a feed of %lld", (long long)S);
        EXPECT(hipstub_launches_of("k_ppc_partial") == p0 + 3, "three sub-batches (%ld launches)", hipstub_launches_of("k_ppc_partial") - p0);
        const long m0 = hipstub_mallocs();
        p0 = hipstub_launches_of("k_ppc_partial");
        EXPECT(lr_ppc_accumulate(h, dev.p, 3000, 1, nullptr) == LR_OK && hipstub_mallocs() == m0, "a longer feed allocates nothing: the workspace does not grow with S");
        int64_t want = 0;  // from s = S + 1: every sub-batch ends at the last multiple of 4 within `sub` draws, or with the feed
        for (int64_t b = S + 1, end = S + 1 + 3000; b < end; ++want) b = std::min(end, (b + sub) & ~int64_t(3));
        EXPECT(hipstub_launches_of("k_ppc_partial") == p0 + want, "%lld sub-batches (%ld launches)", (long long)want, hipstub_launches_of("k_ppc_partial") - p0);
        lr_ppc_destroy(h);
        lr_model_destroy(m);
    }
}

static void errors() {
    Design keep;
    lr_model* m = model(LR_F32, 5, 50, 1.0, false, &keep);
    lr_ppc* h = nullptr;
    std::vector<int32_t> g = labels(50, 3);
    std::vector<float> draws((size_t)64 * 5, 0.f);
    std::vector<int32_t> c(64 * 3);
    std::vector<double> d(128);
    auto refused = [&](int rc, const char* word) { return rc == LR_ERR_INVALID && std::strstr(lr_last_error(), word) != nullptr; };
    const long mallocs = hipstub_mallocs(), launches = hipstub_launches();
    EXPECT(refused(lr_ppc_create(nullptr, nullptr, nullptr, 50, nullptr, 1, 0, &h), "NULL") && refused(lr_ppc_create(m, nullptr, nullptr, 50, nullptr, 1, 0, nullptr), "NULL"),
           "NULL model / out");
    EXPECT(refused(lr_ppc_create(m, nullptr, nullptr, 0, nullptr, 1, 0, &h), "positive") && refused(lr_ppc_create(m, nullptr, nullptr, -4, nullptr, 1, 0, &h), "positive"), "r <= 0");
    EXPECT(refused(lr_ppc_create(m, nullptr, nullptr, 49, nullptr, 1, 0, &h), "own 50 rows") && refused(lr_ppc_create(m, nullptr, keep.y.data(), 50, nullptr, 1, 0, &h), "y_new without"),
           "r != n, y_new without X_new");
    EXPECT(refused(lr_ppc_create(m, nullptr, nullptr, 50, g.data(), 0, 0, &h), "G must be") && refused(lr_ppc_create(m, nullptr, nullptr, 50, g.data(), 33, 0, &h), "G must be") &&
               refused(lr_ppc_create(m, nullptr, nullptr, 50, nullptr, 2, 0, &h), "one group"), "G outside 1 .. 32, G without labels");
    EXPECT(refused(lr_ppc_create(m, nullptr, nullptr, 50, g.data(), 2, 0, &h), "groups[2]=2 is outside"), "a group label >= G");
    g[7] = -1;
    EXPECT(refused(lr_ppc_create(m, nullptr, nullptr, 50, g.data(), 3, 0, &h), "groups[7]=-1 is outside"), "a negative group label");
    g[7] = 1;
    for (double bad : {(double)INFINITY, (double)NAN}) {
        const double was = keep.X[3 * 5 + 2];
        keep.X[3 * 5 + 2] = bad;
        EXPECT(refused(lr_ppc_create(m, keep.X.data(), keep.y.data(), 50, nullptr, 1, 0, &h), "X_new[3,2] is not finite"), "X_new = %g", bad);
        keep.X[3 * 5 + 2] = was;
    }
    keep.y[9] = 0.5;
    EXPECT(refused(lr_ppc_create(m, keep.X.data(), keep.y.data(), 50, nullptr, 1, 0, &h), "y_new[9]=0.5 is not 0/1"), "a label outside {0, 1}");
    keep.y[9] = 1.0;
    EXPECT(h == nullptr && hipstub_mallocs() == mallocs && hipstub_launches() == launches, "refused ahead of any device access (%ld allocations, %ld launches)",
           hipstub_mallocs() - mallocs, hipstub_launches() - launches);
    EXPECT(lr_ppc_create(m, nullptr, nullptr, 50, g.data(), 3, 0, &h) == LR_OK && h, "create");
    const long mallocs1 = hipstub_mallocs(), launches1 = hipstub_launches();
    EXPECT(refused(lr_ppc_accumulate(nullptr, draws.data(), 2, 0, nullptr), "NULL") && refused(lr_ppc_accumulate(h, nullptr, 2, 0, nullptr), "NULL") &&
               refused(lr_ppc_accumulate(h, draws.data(), 0, 0, nullptr), "positive"), "NULL accumulator / draws, S <= 0");
    EXPECT(refused(lr_ppc_terms(nullptr, draws.data(), 2, 0, 0, nullptr, c.data(), d.data(), nullptr), "NULL") &&
               refused(lr_ppc_terms(h, nullptr, 2, 0, 0, nullptr, c.data(), d.data(), nullptr), "NULL") &&
               refused(lr_ppc_terms(h, draws.data(), 2, 0, 0, nullptr, nullptr, d.data(), nullptr), "NULL") &&
               refused(lr_ppc_terms(h, draws.data(), 2, 0, 0, nullptr, c.data(), nullptr, nullptr), "NULL") &&
               refused(lr_ppc_terms(h, draws.data(), 0, 0, 0, nullptr, c.data(), d.data(), nullptr), "positive") &&
               refused(lr_ppc_terms(h, draws.data(), 2, -1, 0, nullptr, c.data(), d.data(), nullptr), "first_index"), "terms arguments");
    EXPECT(refused(lr_ppc_result(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL") && refused(lr_ppc_reset(nullptr), "NULL"), "NULL result / reset");
    EXPECT(hipstub_mallocs() == mallocs1 && hipstub_launches() == launches1, "refused ahead of any device access");
    lr_ppc_destroy(h);
    lr_ppc_destroy(nullptr);
    lr_model_destroy(m);
}

int main() {
    const std::vector<unsigned char> zeros((size_t)3000 * 128 * 8, 0);  // zero-filled draws for everything below
    void* stream = nullptr;
    EXPECT(lr_stream_create(0, &stream) == LR_OK, "stream");
    for (int dtype : {LR_F32, LR_F64})
        for (const Shape& s : {Shape{dtype, 5, 50, 1}, Shape{dtype, 8, 50, 3}, Shape{dtype, 100, 20, 32}, Shape{dtype, 3, 1300, 7}, Shape{dtype, 1, 1, 1}}) {
            life(s, zeros.data(), stream);
            failing_allocations(s, zeros.data());
        }
    sub_batches();
    errors();
    EXPECT(lr_stream_destroy(0, stream) == LR_OK, "stream destroy");
    return finish("ppc harness", "k_ppc_partial");
}
