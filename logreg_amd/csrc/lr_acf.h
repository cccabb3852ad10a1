// lr_acf.h -- the streaming autocorrelation / Geyer-ESS accumulator of include/logreg_hip_acf.h: blocks [k][C][p] of draws in time
// order -> per series (chain, coordinate) the lag sums S_l = sum_t xs_t xs_{t-l}, l = 0..K, of the pivoted values xs_t = x_t - x_0,
// and from them the autocovariance, the pair scan and the effective sample size.
//
// State, per series s = c p + j of the flattened [C p] axis (NS series), all float64:
//     S [NS][K+1]   lag sums            total [NS]   sum of xs            x0 [NS]   the pivot (the series' first value)
//     head [NS][K]  the first K xs      tail [NS][K] the last K xs, oldest first; zero where the series has no value (yet)
//
// k_acf_accumulate.  A workgroup takes kAcfTile consecutive series (a time row is read in segments of 64 / 128 bytes) and walks the
// block in tiles of kAcfSteps time steps.  Per series LDS holds [pad | last K | new steps] as xs.  One wave owns one series at a time,
// lane = lag (a lane owns lags l, l + 64, ... when K > 63, in registers -- the slot loop is unrolled, nothing is indexed
// dynamically).  Per time step: xs_t is a broadcast read (eight steps at a time, as 16-byte reads), xs_{t-l} a read of consecutive
// doubles, and S_l = fma(xs_t, xs_{t-l}, S_l): ONE fma per (t, l), in t order, whatever the tiling and however the draws were cut
// into calls -- the lag sums are the same bytes for every chunking.  Steps before the series began read the zeros of the tail:
// fma(x, 0, S) = S exactly (S is +0 until the first real term).  The total is the same kind of sum: one add per t in t order.
// Nothing is padded with dummy steps (an fma with a zero factor can flip the sign of a zero sum).
//
// k_acf_finish.  One thread per series: acov[l] = (S_l - ms (H_l + T_l) + (n - l) ms^2) / n with ms = total / n, H_l = total - (sum of
// the last l), T_l = total - (sum of the first l); rho, the pair scan, ESS; every product spelled as fma.  A series whose total or S_0
// is not finite held a NaN or an inf (or overflowed): its ESS and acov are NaN.  It writes V [K+4][NS] (rows as the result table's).
// k_acf_partial / k_acf_final sum V over the chains: a fixed tree inside a workgroup of 256 chains, the workgroups in order.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lr {

constexpr int kAcfMaxLag = 255;
constexpr int kAcfTile = 16;    // series per workgroup
constexpr int kAcfBlock = 256;  // 4 waves
constexpr int kAcfSteps = 128;  // time steps staged at a time
constexpr int kAcfHeadRows = 3; // rows of V ahead of the autocovariances: ESS, capped, NaN

// doubles per series in LDS: pad + last K + new steps (+ 2: the rows of a tile start 4 banks apart).  Even, as K + 1 is: the new steps
// of every series start on a 16-byte boundary.
__host__ __device__ inline int acf_row_doubles(int K) { return K + 1 + kAcfSteps + 2; }

template <typename T, int NL>
__global__ void __launch_bounds__(kAcfBlock) k_acf_accumulate(const T* __restrict__ block, int64_t k, int64_t NS, int K, int64_t n0,
                                                              double* __restrict__ S, double* __restrict__ total, double* __restrict__ x0,
                                                              double* __restrict__ head, double* __restrict__ tail) {
    extern __shared__ __attribute__((aligned(16))) double w[];  // [kAcfTile][W]
    const int W = acf_row_doubles(K);
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * kAcfTile;
    const int ns = NS - s0 < kAcfTile ? (int)(NS - s0) : kAcfTile;
    const int sl = tid % kAcfTile, tl = tid / kAcfTile;  // staging: this thread's series and its first time row
    const bool live = sl < ns;
    double piv = 0.0;
    if (live) {
        piv = n0 == 0 ? (double)block[s0 + sl] : x0[s0 + sl];
        if (n0 == 0 && tl == 0) x0[s0 + sl] = piv;
    }
    for (int i = tid; i < ns * K; i += kAcfBlock) w[(i / K) * W + 1 + i % K] = tail[s0 * K + i];

    const int wave = tid / 64, lane = tid % 64;
    for (int64_t t0 = 0; t0 < k; t0 += kAcfSteps) {
        const int kt = k - t0 < kAcfSteps ? (int)(k - t0) : kAcfSteps;
        if (live) {
            for (int t = tl; t < kt; t += kAcfBlock / kAcfTile) {
                const double v = (double)block[(t0 + t) * NS + s0 + sl] - piv;
                w[sl * W + K + 1 + t] = v;
                const int64_t tg = n0 + t0 + t;
                if (tg < K) head[(s0 + sl) * K + tg] = v;
            }
        }
        __syncthreads();
        for (int s = wave; s < ns; s += kAcfBlock / 64) {
            double* ws = w + s * W;
            const double* xn = ws + K + 1;  // the new steps
            double* Srow = S + (s0 + s) * (K + 1);
            double acc[NL];
            const double* hist[NL];  // hist[j][t] = xs_{t - lag}
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int lag = lane + 64 * j < K ? lane + 64 * j : K;  // lanes past the last lag redo it and store nothing
                hist[j] = xn - lag;
                acc[j] = Srow[lag];
            }
            double tot = total[s0 + s];
            int t = 0;
            for (; t + 8 <= kt; t += 8) {
                double x[8];
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    const double2 v = *reinterpret_cast<const double2*>(xn + t + i);
                    x[i] = v.x;
                    x[i + 1] = v.y;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) tot += x[i];
#pragma unroll
                for (int j = 0; j < NL; ++j)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[j] = __builtin_fma(x[i], hist[j][t + i], acc[j]);
            }
            for (; t < kt; ++t) {
                const double x = xn[t];
                tot += x;
#pragma unroll
                for (int j = 0; j < NL; ++j) acc[j] = __builtin_fma(x, hist[j][t], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (lane + 64 * j <= K) Srow[lane + 64 * j] = acc[j];
            if (lane == 0) total[s0 + s] = tot;
            // the last K values move to the front of the row: this wave's own row, reads ahead of writes
            double keep[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) keep[j] = lane + 64 * j < K ? ws[1 + kt + lane + 64 * j] : 0.0;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (lane + 64 * j < K) ws[1 + lane + 64 * j] = keep[j];
        }
        __syncthreads();
    }
    for (int i = tid; i < ns * K; i += kAcfBlock) tail[s0 * K + i] = w[(i / K) * W + 1 + i % K];
}

// V [kAcfHeadRows + K + 1][NS]: row 0 ESS, row 1 capped (0 / 1), row 2 NaN (0 / 1), row 3 + l acov[l]
__global__ void __launch_bounds__(256) k_acf_finish(int64_t NS, int K, int64_t n, const double* __restrict__ S, const double* __restrict__ total,
                                                    const double* __restrict__ head, const double* __restrict__ tail, double* __restrict__ V) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= NS) return;
    const double nd = (double)n;
    const double* Srow = S + s * (K + 1);
    const double* hrow = head + s * K;
    const double* trow = tail + s * K;
    const double tot = total[s];
    const bool bad = !(__builtin_isfinite(tot) && __builtin_isfinite(Srow[0]));
    const double m = tot / nd;
    const int64_t pairs = (K + 1) / 2 < n / 2 ? (K + 1) / 2 : n / 2;
    double first = 0.0, last = 0.0;  // sums of the first l / the last l values
    double acov0 = 0.0, even = 0.0, sum = 0.0;
    bool scan = false, stopped = false;
    for (int l = 0; l <= K; ++l) {
        double a = 0.0;
        if (bad) {
            a = __builtin_nan("");
        } else if (l < n) {
            const double c = (tot - last) + (tot - first);
            const double v = __builtin_fma(-m, c, Srow[l]);
            const double nm = (double)(n - l) * m;
            a = __builtin_fma(nm, m, v) / nd;
        }
        V[(kAcfHeadRows + l) * NS + s] = a;
        if (l == 0) {
            acov0 = a;
            scan = !bad && n >= 4 && a > 0.0;
        }
        if (l < K) {
            first += hrow[l];
            last += trow[K - 1 - l];
        }
        if (scan && !stopped) {
            const double rho = a / acov0;
            if ((l & 1) == 0) {
                even = rho;
            } else if (l / 2 < pairs) {
                const double g = even + rho;
                if (g <= 0.0) stopped = true;
                else sum += g;
            }
        }
    }
    double ess = nd, capped = 0.0;
    if (bad) {
        ess = __builtin_nan("");
    } else if (scan) {
        const double tau = __builtin_fma(2.0, sum, -1.0);
        if (tau > 0.0) ess = nd / tau;
        if (!stopped && (K + 1) / 2 < n / 2) capped = 1.0;
    }
    V[s] = ess;
    V[NS + s] = capped;
    V[2 * NS + s] = bad ? 1.0 : 0.0;
}

// grid (ceil(C / 256), rows): a fixed tree over the 256 chains of a workgroup, per coordinate.  part [gridDim.x][rows][p]
__global__ void __launch_bounds__(256) k_acf_partial(const double* __restrict__ V, int64_t C, int p, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t NS = C * p, c = (int64_t)blockIdx.x * 256 + tid;
    const int64_t r = blockIdx.y, rows = gridDim.y;
    for (int j = 0; j < p; ++j) {
        red[tid] = c < C ? V[r * NS + c * p + j] : 0.0;
        __syncthreads();
        for (int half = 128; half >= 1; half >>= 1) {
            if (tid < half) red[tid] += red[tid + half];
            __syncthreads();
        }
        if (tid == 0) part[((int64_t)blockIdx.x * rows + r) * p + j] = red[0];
        __syncthreads();
    }
}

// one thread per (row, coordinate): the workgroups' partials summed in workgroup order
__global__ void __launch_bounds__(256) k_acf_final(const double* __restrict__ part, int64_t nblocks, int64_t cells, double* __restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    double s = part[e];
    for (int64_t b = 1; b < nblocks; ++b) s += part[b * cells + e];
    sums[e] = s;
}

}  // namespace lr
