// harness.h -- TEST INFRASTRUCTURE: what the stand-alone harnesses of tests/host/ share.  Each is a program of its own that drives the
// C ABI on the stub HIP runtime (hip_stub.cpp: kernel launches are validated no-ops, device memory is the host heap) and is built
// under the sanitizers by tests/host_build.py.  Here: the failure count and EXPECT, a device buffer, the synthetic model, the option
// blocks, the bracket that makes one device allocation fail, and the closing checks with the summary line the tests read.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "hip_stub.h"
#include "logreg_hip.h"
#include "logreg_hip_adapt.h"

inline int g_fail = 0;
#define EXPECT(cond, ...)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s  -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                      \
            std::printf("  (last error: %s)\n", lr_last_error());          \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

struct Dev {  // a device buffer through the ABI's own allocator
    void* p = nullptr;
    explicit Dev(size_t bytes) { if (lr_malloc(0, bytes, &p) != LR_OK) p = nullptr; }
    ~Dev() { if (p) lr_free(0, p); }
};

// The nth device allocation from here (1 = the next) fails, once; leaving the scope disarms it on every path.
struct FailMallocAt {
    explicit FailMallocAt(long nth) { hipstub_fail_malloc_at(nth); }
    ~FailMallocAt() { hipstub_fail_malloc_at(-1); }
    FailMallocAt(const FailMallocAt&) = delete;
    FailMallocAt& operator=(const FailMallocAt&) = delete;
};

struct Design { std::vector<double> X, y; };  // what model() was made from, for a caller that reads it afterwards

// A model on a small synthetic design: an intercept and p - 1 columns on a 13-point lattice, labels 1 on odd rows (on every third
// row from row 0 with thirds), a N(0, prior_sd^2) prior on every coefficient.
inline lr_model* model(int dtype, int p, int64_t n = 50, double prior_sd = 1.0, bool thirds = false, Design* keep = nullptr) {
    Design d;
    d.X.resize((size_t)n * p);
    d.y.resize((size_t)n);
    const std::vector<double> sd((size_t)p, prior_sd);
    for (int64_t i = 0; i < n; ++i) {
        d.y[i] = thirds ? (double)(i % 3 == 0) : (double)(i & 1);
        for (int j = 0; j < p; ++j) d.X[i * p + j] = j == 0 ? 1.0 : 0.01 * (double)((i * 7 + j * 3) % 13) - 0.06;
    }
    lr_model* m = nullptr;
    EXPECT(lr_model_create(d.X.data(), d.y.data(), n, p, sd.data(), dtype, 0, &m) == LR_OK && m, "model (dtype %d, p %d, n %lld)", dtype, p, (long long)n);
    if (keep) *keep = std::move(d);
    return m;
}

inline lr_run_opts run_opts(int64_t C, int on_device = 0, void* stream = nullptr, int64_t iters = 1, int mode = LR_MODE_AUTO) {
    lr_run_opts o;
    std::memset(&o, 0, sizeof(o));
    o.n_chains = C;
    o.thin = 1;
    o.iters = iters;
    o.seed = 9;
    o.mode = mode;
    o.on_device = on_device;
    o.stream = stream;
    return o;
}

inline lr_adapt_opts adapt_opts(int W, int adapt_metric = 1, double eps0 = 0.0) {
    lr_adapt_opts o;
    std::memset(&o, 0, sizeof(o));
    o.W = W;
    o.adapt_metric = adapt_metric;
    o.eps0 = eps0;
    return o;
}

// The closing checks of a harness and its summary line; -> the exit status.  `kernel`: the one whose launches the line counts, or NULL.
inline int finish(const char* name, const char* kernel) {
    EXPECT(hipstub_live_allocs() == 0 && hipstub_live_streams() == 0, "%ld device buffers, %ld streams left", hipstub_live_allocs(), hipstub_live_streams());
    EXPECT(hipstub_bad_launches() == 0 && hipstub_bad_waits() == 0 && hipstub_wrong_device() == 0, "%ld bad launches, %ld bad waits, %ld on the wrong device", hipstub_bad_launches(),
           hipstub_bad_waits(), hipstub_wrong_device());
    std::printf("%s: %ld kernel launches", name, hipstub_launches());
    if (kernel) std::printf(" (%ld %s)", hipstub_launches_of(kernel), kernel);
    std::printf(", %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
