// lr_dense_adapt.h -- the pooled p x p co-moment of the dense-metric warm-up (include/logreg_hip_dense.h "Warm-up"): in a metric window
// every iteration's states of all chains enter one pooled (n, mean [p], M [p][p]) over chains and time, M_jl = sum (x_j - mean_j)(x_l -
// mean_l).  Two kernels per window iteration, behind k_adapt_partial / ahead of k_adapt_update (lr_adapt.h), whose definitions they extend
// from the variance of a coordinate to the co-moment of a pair -- the diagonal M_jj IS that M2_j, operation for operation:
//     k_dense_comoment_partial   one workgroup per 256 chains: mean_b [P] as k_adapt_partial forms it, then for every pair l <= j
//                                e[q] = fma(d_ij, d_il, e[q]) over i = q, q + Q, ... (ascending), the same halving tree over q
//     k_dense_comoment_merge     one workgroup, one lane per pair: the Chan merge of the workgroups' triples in workgroup order, then of the
//                                iteration's triple INTO the window's (an empty window takes it as it is)
//         n = n_a + n_b, d = mean_b - mean_a:  M_jl = fma(d_j * d_l, n_a * n_b / n, M_a_jl + M_b_jl),  mean_j = fma(d_j, n_b / n, mean_a_j)
// Everything float64, nothing contracted, no atomics.  The window's end (S = M / (n - 1), the regularised Sigma, its factorisation) is the
// host's: lr_api.hip dense_window_end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_adapt.h"

namespace lr {

// a triple: n | mean [P] | M [P][P] (row-major; the lower triangle l <= j is kept)
__host__ __device__ constexpr int dense_triple_words(int P) { return 1 + P + P * P; }

template <typename T, int P>
__global__ void __launch_bounds__(kAdaptBlock) k_dense_comoment_partial(const T* __restrict__ x, int64_t C, int p, double* __restrict__ partial) {
#pragma clang fp contract(off)
    static_assert(P >= 4 && P <= 32 && kAdaptBlock % P == 0, "lane map");
    constexpr int Q = kAdaptBlock / P;
    __shared__ double v[kAdaptBlock];
    __shared__ double mu[P];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kAdaptBlock;
    const int nb = C - c0 < kAdaptBlock ? (int)(C - c0) : kAdaptBlock;
    double* out = partial + (size_t)blockIdx.x * dense_triple_words(P);
    const int j = tid % P, q = tid / P;
    const bool real = j < p;
    double s1 = 0.0;
    if (real)
        for (int i = q; i < nb; i += Q) s1 += (double)x[(c0 + i) * p + j];
    v[tid] = s1;
    __syncthreads();
    for (int s = Q / 2; s > 0; s >>= 1) {
        if (q < s) v[tid] += v[tid + s * P];
        __syncthreads();
    }
    if (tid < P) {
        mu[tid] = v[tid] / (double)nb;
        out[1 + tid] = mu[tid];
    }
    if (tid == 0) out[0] = (double)nb;
    __syncthreads();
    const double mean_j = mu[j];
    for (int l = 0; l < p; ++l) {  // the pair (j, l) in the lanes of coordinate j >= l
        const double mean_l = mu[l];
        double s2 = 0.0;
        if (real && l <= j)
            for (int i = q; i < nb; i += Q) {
                const double dj = (double)x[(c0 + i) * p + j] - mean_j, dl = (double)x[(c0 + i) * p + l] - mean_l;
                s2 = __builtin_fma(dj, dl, s2);
            }
        v[tid] = s2;
        __syncthreads();
        for (int s = Q / 2; s > 0; s >>= 1) {
            if (q < s) v[tid] += v[tid + s * P];
            __syncthreads();
        }
        if (tid < P && l <= tid) out[1 + P + tid * P + l] = v[tid];
        __syncthreads();
    }
}

// win: the window's triple (n = 0: empty); lane (j, l), l <= j < p
template <int P>
__global__ void __launch_bounds__(P * P < 64 ? 64 : P * P) k_dense_comoment_merge(const double* __restrict__ partial, int64_t B, int p, double* __restrict__ win) {
#pragma clang fp contract(off)
    constexpr int TW = dense_triple_words(P);
    const int j = threadIdx.x / P, l = threadIdx.x % P;
    const bool mine = threadIdx.x < P * P && j < p && l <= j;
    double n = 0.0, mj = 0.0, ml = 0.0, M = 0.0;
    auto merge = [&](double nb, double bj, double bl, double Mb) {  // (n, mj, ml, M) <- (nb, bj, bl, Mb), both counts > 0
        const double nn = n + nb, dj = bj - mj, dl = bl - ml;
        M = __builtin_fma(dj * dl, n * nb / nn, M + Mb);
        mj = __builtin_fma(dj, nb / nn, mj);
        ml = __builtin_fma(dl, nb / nn, ml);
        n = nn;
    };
    if (mine) {
        n = partial[0];
        mj = partial[1 + j];
        ml = partial[1 + l];
        M = partial[1 + P + j * P + l];
        for (int64_t b = 1; b < B; ++b) {
            const double* pb = partial + b * TW;
            merge(pb[0], pb[1 + j], pb[1 + l], pb[1 + P + j * P + l]);
        }
        const double wn = win[0];
        if (wn > 0.0) {
            const double in = n, ij = mj, il = ml, iM = M;
            n = wn;
            mj = win[1 + j];
            ml = win[1 + l];
            M = win[1 + P + j * P + l];
            merge(in, ij, il, iM);
        }
    }
    __syncthreads();  // every lane has read win[0] and the means it needs before any lane stores (one workgroup)
    if (mine) {
        win[1 + P + j * P + l] = M;
        if (l == j) win[1 + j] = mj;
        if (threadIdx.x == 0) win[0] = n;
    }
}

}  // namespace lr
