// lr_hs.h -- the fused many-chain horseshoe Polya-Gamma Gibbs sampler (include/logreg_hip_hs.h: the model, the sweep, the random stream,
// the order of every sum).
//
// k_hs is k_pg's sweep (lr_pg.h pg_sweeps: phases 1 and 2, the factorisation, the solves, the skip rule, the streaming statistics) with the
// three hooks of HsState: the prior precision on the diagonal of A gains s_j / (tau^2 lambda_j^2), the scales are redrawn after the
// back-solve, when A is dead, and a kept draw may write them out.  Lane r of a chain's 16 owns coordinates r + 16 k, as it owns them in
// k_pg, so the local scales need no exchange; the global scale needs two group_sum<16> (the quadratic form, the Gamma variate).
//
// Where the hyper-state lives: tau^2 and xi are replicated in registers of the 16 lanes; lambda_j^2 and nu_j stay in the `hyper` array in
// global memory between their uses (one load at the diagonal, one load and one store per coordinate in the hyper-step, always by the lane
// that owns the coordinate).  k_pg<double, 32> holds 496 of the 512 registers of a lane, so there is no room to carry them over phase 2.
// No LDS beyond k_pg's, no runtime-indexed register array, every loop has a compile-time bound, no comparison lets a NaN through.
#pragma once

#include "lr_pg.h"

namespace lr {

constexpr uint32_t TAG_HS = 0x02000000u;  // | b: block b of the hyper-step (LR_HS_TAG)
constexpr uint32_t kHsBlockGlobal = 32, kHsBlockGamma = 33;  // E3 and z; the exponentials of G, two per block (LR_HS_BLOCK_*)
constexpr double kHsLo = 1e-100, kHsHi = 1e100;              // LR_HS_MIN, LR_HS_MAX

template <typename T, int P> struct HsArgs {
    PgArgs<T, P> pg;         // omega_out is null; pg.counters is an lr_hs_counters array (`reserved` is `clamped`)
    const double* hyper_in;  // [C][2 p + 2]: lambda^2 [p], nu [p], tau^2, xi
    double* hyper_out;       // a run: the same array; lr_hs_hyper: its output
    double* scale_out;       // [iters][C][p + 1] or null
    double inv_tau0sq;       // 1 / tau0^2
    uint32_t shrink;         // bit j: coordinate j is shrunk
    int nexp, odd;           // G = E_0 + ... + E_{nexp - 1} (+ z^2 / 2 if odd): nexp = (m + 1) / 2, odd = (m + 1) & 1
    int hyper_only;          // lr_hs_hyper: steps 5-7 of ONE iteration on pg.state, nothing else
};

// E = -ln u, u the 53-bit uniform of two words
__device__ __forceinline__ double hs_expo(uint32_t wa, uint32_t wb) {
    const double u = (((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) + 0.5) * 0x1p-53;
    return -log(u);
}
// one Box-Muller normal from two words, 32-bit uniforms (only its square is used)
__device__ __forceinline__ double hs_normal(uint32_t wa, uint32_t wb) {
    const double ua = ((double)wa + 0.5) * 0x1p-32, ub = ((double)wb + 0.5) * 0x1p-32;
    return sqrt(-2.0 * log(ua)) * cospi(2.0 * ub);
}
// step 7: into [kHsLo, kHsHi]; a NaN leaves `old`; either way n gains 1
__device__ __forceinline__ double hs_clamp(double v, double old, uint32_t& n) {
    const bool nan = !(v == v), lo = v < kHsLo, hi = v > kHsHi;
    n += (nan || lo || hi) ? 1u : 0u;
    return nan ? old : (lo ? kHsLo : (hi ? kHsHi : v));
}
// a value of the caller's hyper array as the sweep reads it (the host entry points refuse what this would change; device memory is
// not read on the host)
__device__ __forceinline__ double hs_sane(double v) {
    uint32_t unused = 0;
    return hs_clamp(v, 1.0, unused);
}

template <typename T, int P> struct HsState {
    static constexpr bool kHyper = true;
    static constexpr int NK = (P + 15) / 16;
    const HsArgs<T, P>& a;
    int r;
    int64_t chain;
    bool live;
    uint64_t gchain;
    double tau2, xi;
    uint32_t clamp_own = 0, clamp_all = 0;  // clamps of this lane's coordinates; of tau^2 and xi (the same in all 16 lanes)

    __device__ __forceinline__ explicit HsState(const HsArgs<T, P>& args) : a(args) {
        r = threadIdx.x & 15;
        chain = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 16;
        live = chain < a.pg.C;
        if (!live) chain = a.pg.C - 1;  // (as pg_sweeps: whole waves stay converged)
        gchain = (uint64_t)(a.pg.chain_offset + chain);
        const double* h = a.hyper_in + chain * (2 * (int64_t)a.pg.p + 2);
        tau2 = hs_sane(h[2 * a.pg.p]);
        xi = hs_sane(h[2 * a.pg.p + 1]);
    }
    __device__ __forceinline__ double shrunk(int j) const { return j < a.pg.p ? (double)((a.shrink >> j) & 1u) : 0.0; }

    // step 2: the prior precision of coordinate r + 16 k
    __device__ __forceinline__ double precision(int k, double ivar) const {
        const int j = r + 16 * k;
        const double l2 = hs_sane(a.hyper_out[chain * (2 * (int64_t)a.pg.p + 2) + (j < a.pg.p ? j : 0)]);
        return ivar + shrunk(j) * ((1.0 / tau2) * (1.0 / l2));
    }

    // steps 5-7 for iteration `iter` at the state x; a skipped sweep leaves everything in place
    __device__ __forceinline__ void step(bool skip, const T (&x)[NK], uint64_t iter) { update(skip, x, iter, a.hyper_out); }

    __device__ __forceinline__ void update(bool skip, const T (&x)[NK], uint64_t iter, const double* from) {
        const int p = a.pg.p;
        const uint32_t c0 = (uint32_t)gchain, c1 = (uint32_t)iter, c2 = (uint32_t)(iter >> 32), k0 = (uint32_t)a.pg.seed, k1 = (uint32_t)(a.pg.seed >> 32);
        const double* hin = from + chain * (2 * (int64_t)p + 2);
        double* hout = a.hyper_out + chain * (2 * (int64_t)p + 2);
        const double half_it2 = 0.5 * (1.0 / tau2);
        double part = 0.0;
        uint32_t nc = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = r + 16 * k, js = j < p ? j : 0;
            const bool on = shrunk(j) != 0.0;
            const double l_old = hs_sane(hin[js]), n_old = hs_sane(hin[p + js]);
            const U4 w = philox4x32_10(c0, c1, c2, TAG_HS | (uint32_t)j, k0, k1);
            const double b2 = (double)x[k] * (double)x[k];
            uint32_t c = 0;
            const double l_new = hs_clamp((1.0 / n_old + b2 * half_it2) / hs_expo(w.x, w.y), l_old, c);
            const double il = 1.0 / l_new;
            const double n_new = hs_clamp((1.0 + il) / hs_expo(w.z, w.w), n_old, c);
            part += on ? b2 * il : 0.0;
            nc += on ? c : 0u;
            if (j < p && live && !skip) {
                hout[j] = on ? l_new : l_old;
                hout[p + j] = on ? n_new : n_old;
            }
        }
        const double quad = group_sum<16>(part);
        // G: lane r draws E_r
        const U4 wg = philox4x32_10(c0, c1, c2, TAG_HS | (kHsBlockGamma + (uint32_t)(r >> 1)), k0, k1);
        const double e = (r & 1) ? hs_expo(wg.z, wg.w) : hs_expo(wg.x, wg.y);
        const U4 w3 = philox4x32_10(c0, c1, c2, TAG_HS | kHsBlockGlobal, k0, k1);
        const double z = hs_normal(w3.z, w3.w);
        const double g = group_sum<16>(r < a.nexp ? e : 0.0) + (a.odd ? 0.5 * (z * z) : 0.0);
        uint32_t ca = 0;
        const double t_new = hs_clamp((1.0 / xi + 0.5 * quad) / g, tau2, ca);
        const double x_new = hs_clamp((a.inv_tau0sq + 1.0 / t_new) / hs_expo(w3.x, w3.y), xi, ca);
        tau2 = skip ? tau2 : t_new;
        xi = skip ? xi : x_new;
        clamp_own += skip ? 0u : nc;
        clamp_all += skip ? 0u : ca;
    }

    // a kept draw: lambda_j^2 (1 where unshrunk) and tau^2
    __device__ __forceinline__ void keep(int64_t it) const {
        if (!a.scale_out) return;
        const int p = a.pg.p;
        double* o = a.scale_out + (it * a.pg.C + chain) * (p + 1);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = r + 16 * k;
            if (j < p) o[j] = shrunk(j) != 0.0 ? hs_sane(a.hyper_out[chain * (2 * (int64_t)p + 2) + j]) : 1.0;
        }
        if (r == 0) o[p] = tau2;
    }

    // tau^2, xi and the clamp count of the launch
    __device__ __forceinline__ void finish() {
        const double own = group_sum<16>((double)clamp_own);
        if (live && r == 0) {
            double* h = a.hyper_out + chain * (2 * (int64_t)a.pg.p + 2);
            h[2 * a.pg.p] = tau2;
            h[2 * a.pg.p + 1] = xi;
            if (a.pg.counters) a.pg.counters[chain].reserved += (uint32_t)own + clamp_all;
        }
    }
};

template <typename T, int P>
__global__ void __launch_bounds__(256) k_hs(ModelArgs<T, P> m, HsArgs<T, P> a) {
    HsState<T, P> h(a);
    if (a.hyper_only) {
        constexpr int NK = HsState<T, P>::NK;
        T x[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) x[k] = h.r + 16 * k < a.pg.p ? a.pg.state[h.chain * a.pg.p + h.r + 16 * k] : T(0);
        h.update(false, x, (uint64_t)a.pg.iter_offset, a.hyper_in);
    } else {
        pg_sweeps<T, P>(m, a.pg, h);
    }
    h.finish();
}

}  // namespace lr
