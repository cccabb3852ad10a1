// lr_adapt.h -- the two kernels that turn one warm-up iteration of all chains into the next iteration's step size and metric
// (include/logreg_hip_adapt.h states the arithmetic line by line; this file is that text as code).  Per iteration, on one stream:
//     k_nuts<.., TUNED>   one NUTS iteration from the device-resident NutsTune block; writes astat [C]        (lr_nuts.h)
//     k_adapt_partial     one workgroup per 256 chains: sum256 of astat and, in a metric window, (n, mean, M2) per coordinate
//     k_adapt_update      one wave (P = 128: two): merges the partials in workgroup order, the dual-averaging step, the fold into the window's triple,
//                         at a window's end the metric and the restart; writes the next NutsTune block, a trace row, a metric row
// The schedule is known on the host: the iteration index, m and the window flags come in by value (AdaptStep).  Everything is float64,
// nothing contracts (products inside sums are spelled fma), no float atomics; the partials are plain stores in workgroup order.
// On the stepwise engine (include/logreg_hip_adapt_tall.h) the iteration is the launches of k_tall_nuts_update<.., TUNED> (lr_tall_nuts.h) and
// the two kernels run at P = 64 and 128 as well, over the engine's padded states (row stride `ld` = P).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_nuts.h"

namespace lr {

constexpr int kAdaptBlock = 256;
constexpr int kAdaptTraceCols = 5;  // LR_ADAPT_TRACE_COLS
// slots of AdaptDev::da
enum { AD_HBAR = 0, AD_LOG_EPS_BAR, AD_MU, AD_EPS, AD_EPS_REPORT, AD_SKIPPED, AD_WINDOWS, AD_SLOTS };

__host__ __device__ constexpr int adapt_partial_words(int P) { return 2 + 2 * P; }  // sum of astat, n_b, mean_b [P], M2_b [P]

struct AdaptDev {
    double* da;       // [AD_SLOTS]
    double* dmm;      // [p]
    double* win;      // [1 + 2 p]: n, mean [p], M2 [p]
    double* partial;  // [ceil(C / 256)][adapt_partial_words(P)]
    double* trace;    // [W][kAdaptTraceCols]
    double* metric;   // [windows][2][p]
};

struct AdaptStep {
    int64_t C, t;
    int p, m;                  // m: iterations since the last restart, counted from 1
    int window;                // index of the window iteration t lies in, -1 outside
    int window_end, last;      // t is a window's last iteration / the warm-up's
    double delta, gamma, t0, kappa;
};

// (n_a, mean_a, M2_a) <- (n_b, mean_b, M2_b), n_a > 0 and n_b > 0
__device__ __forceinline__ void adapt_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
#pragma clang fp contract(off)
    const double n = na + nb, d = mb - ma;
    ma = __builtin_fma(d, nb / n, ma);
    Ma = __builtin_fma(d * d, na * nb / n, Ma + Mb);
    na = n;
}

// The two kernels' bodies.  Each has two names: k_adapt_* at the fused kernels' widths (P <= 32, both engines) and k_tall_adapt_* at the
// wide ones (P = 64, 128: the stepwise engine only), so that what is instantiated per family can be counted by name.
template <typename T, int P>
__device__ __forceinline__ void adapt_partial(const T* __restrict__ x, int64_t ld, const double* __restrict__ astat, int64_t C, int p, int in_window,
                                              double* __restrict__ partial) {
    // x: the states, row c at x + c ld (ld = p: the caller's [C][p]; ld = P: the stepwise engine's workspace)
#pragma clang fp contract(off)
    static_assert(P >= 4 && P <= 128 && kAdaptBlock % P == 0, "lane map");
    constexpr int Q = kAdaptBlock / P;
    __shared__ double v[kAdaptBlock];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kAdaptBlock;
    const int nb = C - c0 < kAdaptBlock ? (int)(C - c0) : kAdaptBlock;
    double* out = partial + (size_t)blockIdx.x * adapt_partial_words(P);
    v[tid] = tid < nb ? astat[c0 + tid] : 0.0;
    __syncthreads();
    for (int s = kAdaptBlock / 2; s > 0; s >>= 1) {
        if (tid < s) v[tid] += v[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = v[0];
        out[1] = (double)nb;
    }
    if (!in_window) return;  // (the same for every lane)
    __syncthreads();
    const int j = tid % P, q = tid / P;
    const bool real = j < p;
    double s1 = 0.0;
    if (real)
        for (int i = q; i < nb; i += Q) s1 += (double)x[(c0 + i) * ld + j];
    v[tid] = s1;
    __syncthreads();
    for (int s = Q / 2; s > 0; s >>= 1) {
        if (q < s) v[tid] += v[tid + s * P];
        __syncthreads();
    }
    const double mean = v[j] / (double)nb;
    __syncthreads();
    double s2 = 0.0;
    if (real)
        for (int i = q; i < nb; i += Q) {
            const double d = (double)x[(c0 + i) * ld + j] - mean;
            s2 = __builtin_fma(d, d, s2);
        }
    v[tid] = s2;
    __syncthreads();
    for (int s = Q / 2; s > 0; s >>= 1) {
        if (q < s) v[tid] += v[tid + s * P];
        __syncthreads();
    }
    if (tid < P) {
        out[2 + tid] = mean;
        out[2 + P + tid] = v[tid];
    }
}
template <typename T, int P>
__global__ void __launch_bounds__(kAdaptBlock) k_adapt_partial(const T* __restrict__ x, int64_t ld, const double* __restrict__ astat, int64_t C, int p,
                                                                int in_window, double* __restrict__ partial) {
    static_assert(P <= 32, "the wide widths: k_tall_adapt_partial");
    adapt_partial<T, P>(x, ld, astat, C, p, in_window, partial);
}
template <typename T, int P>
__global__ void __launch_bounds__(kAdaptBlock) k_tall_adapt_partial(const T* __restrict__ x, int64_t ld, const double* __restrict__ astat, int64_t C, int p,
                                                                     int in_window, double* __restrict__ partial) {
    static_assert(P > 32, "the fused kernels' widths: k_adapt_partial");
    adapt_partial<T, P>(x, ld, astat, C, p, in_window, partial);
}

// lane = coordinate: one wave, two at P = 128.  What a lane reads that lane 0 writes (d.win[0]) it reads ahead of the one
// __syncthreads(), and lane 0 writes behind it; what lane 0 reads of the others (sh_skip) it reads behind it: the order holds across waves.
__host__ __device__ constexpr int adapt_update_lanes(int P) { return P > 64 ? P : 64; }
template <typename T, int P>
__device__ __forceinline__ void adapt_update(const AdaptDev& d, const AdaptStep& s, NutsTune<T, P>* __restrict__ tune) {
#pragma clang fp contract(off)
    constexpr int PW = adapt_partial_words(P);
    __shared__ double sh_eps;
    __shared__ int sh_skip[P];
    const int j = threadIdx.x;
    const int64_t B = (s.C + kAdaptBlock - 1) / kAdaptBlock;
    const bool mine = j < s.p;
    const bool in_window = s.window >= 0;
    if (j < P) sh_skip[j] = 0;
    const double wn0 = d.win[0];  // the window's count before this iteration (read by every lane ahead of lane 0's store)
    double log_eps_bar = 0.0;
    if (j == 0) {
        double sum = d.partial[0];
        for (int64_t b = 1; b < B; ++b) sum += d.partial[b * PW];
        const double abar = sum / (double)s.C;
        const double m = (double)s.m;
        const double hbar = (1.0 - 1.0 / (m + s.t0)) * d.da[AD_HBAR] + (s.delta - abar) / (m + s.t0);
        const double log_eps = d.da[AD_MU] - sqrt(m) / s.gamma * hbar;
        const double eta = pow(m, -s.kappa);
        log_eps_bar = eta * log_eps + (1.0 - eta) * d.da[AD_LOG_EPS_BAR];
        const double eps = exp(log_eps);
        sh_eps = eps;
        double* row = d.trace + s.t * kAdaptTraceCols;
        row[0] = d.da[AD_EPS];
        row[1] = abar;
        row[2] = log_eps_bar;
        row[3] = (double)s.window;
        row[4] = in_window ? wn0 + (double)s.C : 0.0;
        d.da[AD_HBAR] = s.window_end ? 0.0 : hbar;
        d.da[AD_LOG_EPS_BAR] = s.window_end ? 0.0 : log_eps_bar;
        if (s.window_end) d.da[AD_MU] = log(10.0 * eps);
        d.da[AD_EPS] = eps;
        d.da[AD_EPS_REPORT] = s.last ? exp(log_eps_bar) : eps;
    }
    double dm = mine ? d.dmm[j] : 1.0;
    if (in_window && mine) {
        double n = d.partial[1], mean = d.partial[2 + j], M2 = d.partial[2 + P + j];
        for (int64_t b = 1; b < B; ++b) adapt_merge(n, mean, M2, d.partial[b * PW + 1], d.partial[b * PW + 2 + j], d.partial[b * PW + 2 + P + j]);
        if (wn0 > 0.0) {
            double wn = wn0, wm = d.win[1 + j], wM = d.win[1 + s.p + j];
            adapt_merge(wn, wm, wM, n, mean, M2);
            n = wn;
            mean = wm;
            M2 = wM;
        }
        if (s.window_end) {
            const double var = M2 / (n - 1.0);
            const bool ok = var > 0.0 && var < __builtin_inf();
            if (ok) {
                const double inv = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0));
                dm = 1.0 / inv;
                d.dmm[j] = dm;
            } else {
                sh_skip[j] = 1;
            }
            double* mrow = d.metric + (size_t)s.window * 2 * s.p;
            mrow[j] = var;
            mrow[s.p + j] = dm;
            mean = 0.0;
            M2 = 0.0;
        }
        d.win[1 + j] = mean;
        d.win[1 + s.p + j] = M2;
    }
    __syncthreads();
    if (j == 0) {
        if (in_window) d.win[0] = s.window_end ? 0.0 : wn0 + (double)s.C;
        if (s.window_end) {
            int skipped = 0;
            for (int k = 0; k < s.p; ++k) skipped += sh_skip[k];
            d.da[AD_SKIPPED] += (double)skipped;
            d.da[AD_WINDOWS] += 1.0;
        }
    }
    // the next iteration's tuning, as lr_run_nuts forms it on the host
    const double eps = sh_eps;
    if (j == 0) tune->step = (T)eps;
    if (j < P) {
        tune->a[j] = mine ? (T)sqrt(dm) : T(0);
        tune->b[j] = mine ? (T)(eps / dm) : T(0);
        tune->c[j] = mine ? (T)(1.0 / dm) : T(0);
    }
}
template <typename T, int P>
__global__ void __launch_bounds__(adapt_update_lanes(P)) k_adapt_update(AdaptDev d, AdaptStep s, NutsTune<T, P>* __restrict__ tune) {
    static_assert(P <= 32, "the wide widths: k_tall_adapt_update");
    adapt_update<T, P>(d, s, tune);
}
template <typename T, int P>
__global__ void __launch_bounds__(adapt_update_lanes(P)) k_tall_adapt_update(AdaptDev d, AdaptStep s, NutsTune<T, P>* __restrict__ tune) {
    static_assert(P > 32, "the fused kernels' widths: k_adapt_update");
    adapt_update<T, P>(d, s, tune);
}

}  // namespace lr
