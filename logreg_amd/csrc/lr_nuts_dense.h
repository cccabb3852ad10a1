// lr_nuts_dense.h -- NUTS under a dense metric (include/logreg_hip_dense.h): the tree loop of lr_nuts.h (nuts_run) under
// NutsDenseMetric.  The user's inverse metric Sigma reaches the device factorised by the host (lr_dense.h):
//     s = sqrt(diag Sigma),  R = Sigma / (s s^T) (unit diagonal),  A = L^-T with R = L L^T
// as one block `factor` of 2 P + 2 P P values of T: s [P], 1 / s [P], R [P][P], A [P][P], row-major, zero in padded rows and columns.
//     momentum   p = (A z) / s                  p ~ N(0, Sigma^-1)
//     velocity   v = s o (R (s o p))            = Sigma p;  q += +-eps v
//     kinetic    p . v                          H = -lpost(q) + 1/2 p^T Sigma p
//     U-turn     rho' = rho - (pa + pb) / 2, w = s o (R (s o rho')):  pa . w <= 0 or pb . w <= 0   (one matrix product for both signs)
// R and A live in LDS behind the checkpoints, TRANSPOSED (element [j * P + i] = M[i][j]): in a product lane r reads, for j = 0 .. P - 1
// in ascending order, the element of ITS row i = r + 16 k at [j * P + i] -- the 16 lanes of a row read 16 consecutive words, the four
// chains of a wave the same ones (a broadcast), so no read meets a bank conflict.  The vector is gathered into every lane first
// (dist_gather16 / nuts_gather_small, as `evaluate` gathers the position); each coordinate of a product is computed in exactly one lane
// as one chain of P fma, and every sum over coordinates stays group_sum<16>: every decision is bit-identical in a chain's 16 lanes.
// Per leaf two products (velocity, kinetic energy), one per executed U-turn check, two per iteration for the draw and its energy.
#pragma once

#include "lr_nuts.h"

namespace lr {

template <typename T, int P> struct NutsDenseArgs : NutsArgs<T, P> {  // (a, b, c of NutsArgs are not read)
    const T* factor;  // device memory: s | 1 / s | R | A
};
// TUNED: `step` alone is read from the NutsTune block (the warm-up's step-size adaptation, lr_adapt.h, drives it unchanged); the
// matrices come by argument
template <typename T, int P> struct NutsDenseTunedArgs : NutsDenseArgs<T, P> {
    const NutsTune<T, P>* tune;
    double* astat;
};
template <typename T, int P, bool TUNED> using NutsDenseArgsOf = std::conditional_t<TUNED, NutsDenseTunedArgs<T, P>, NutsDenseArgs<T, P>>;

template <typename T, int P> constexpr size_t nuts_dense_factor_len() { return (size_t)2 * P + (size_t)2 * P * P; }
// LDS of k_nuts_dense beyond the rows and the checkpoints
template <typename T, int P> constexpr size_t nuts_dense_lds_bytes() { return (size_t)2 * P * P * sizeof(T); }

template <typename T, int P, bool TUNED> struct NutsDenseMetric {
    static constexpr int NK = (P + 15) / 16;
    using Args = NutsDenseArgsOf<T, P, TUNED>;
    T sv[NK], siv[NK];
    const T* Rt;  // LDS [P][P] transposed
    const T* At;
    int row[NK];  // the lane's rows (lanes beyond a width < 16 compute row 0 and store zero)
    bool pad;

    __device__ __forceinline__ void load(const Args& a, int r, T* lds) {
        for (int i = threadIdx.x; i < 2 * P * P; i += blockDim.x) {
            const int e = i % (P * P);
            lds[i] = a.factor[2 * P + (i - e) + (e % P) * P + e / P];
        }
        __syncthreads();
        Rt = lds;
        At = lds + P * P;
        pad = r >= P;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = r + 16 * k, js = j < P ? j : 0;
            row[k] = js;
            sv[k] = j < P ? a.factor[js] : T(0);
            siv[k] = j < P ? a.factor[P + js] : T(0);
        }
    }
    // out = M u: the lane's rows, columns in ascending order
    __device__ __forceinline__ void product(const T* Mt, const T (&u)[NK], T (&out)[NK]) const {
        T ub[P];
        if constexpr (P >= 16) {
#pragma unroll
            for (int k = 0; k < NK; ++k) dist_gather16<T, P>(u[k], k, ub);
        } else {
            nuts_gather_small<T, P>(u[0], ub);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < P; ++j) acc = fma_t(Mt[j * P + row[k]], ub[j], acc);
            out[k] = pad ? T(0) : acc;
        }
    }
    // Sigma pm = s o (R (s o pm))
    __device__ __forceinline__ void velocity(const T (&pm)[NK], T (&v)[NK]) const {
        T u[NK], w[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) u[k] = sv[k] * pm[k];
        product(Rt, u, w);
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = sv[k] * w[k];
    }
    __device__ __forceinline__ void momentum(const T (&z)[NK], T (&pm)[NK]) const {
        T w[NK];
        product(At, z, w);
#pragma unroll
        for (int k = 0; k < NK; ++k) pm[k] = w[k] * siv[k];
    }
    __device__ __forceinline__ void drift(bool fwd, T step, const T (&pm)[NK], T (&q)[NK]) const {
        T v[NK];
        velocity(pm, v);
        const T es = fwd ? step : -step;
#pragma unroll
        for (int k = 0; k < NK; ++k) q[k] = fma_t(es, v[k], q[k]);
    }
    __device__ __forceinline__ bool turning(const T (&pa)[NK], const T (&pb)[NK], const T (&rh)[NK]) const {
        T rr[NK], w[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) rr[k] = fma_t(T(-0.5), pa[k] + pb[k], rh[k]);
        velocity(rr, w);
        T sa = T(0), sb = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            sa = fma_t(pa[k], w[k], sa);
            sb = fma_t(pb[k], w[k], sb);
        }
        sa = group_sum<16>(sa);
        sb = group_sum<16>(sb);
        return sa <= T(0) || sb <= T(0);
    }
    __device__ __forceinline__ double kinetic2(const T (&pm)[NK]) const {  // p^T Sigma p
        T v[NK];
        velocity(pm, v);
        T s = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) s = fma_t(pm[k], v[k], s);
        return (double)group_sum<16>(s);
    }
};

template <typename T, int P, int MODE, int R, bool TUNED = false>
__global__ void __launch_bounds__(256) k_nuts_dense(ModelArgs<T, P> m, NutsDenseArgsOf<T, P, TUNED> a) {
    nuts_run<T, P, MODE, R, TUNED, NutsDenseMetric<T, P, TUNED>>(m, a);
}

}  // namespace lr
