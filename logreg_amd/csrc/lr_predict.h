// lr_predict.h -- the streaming posterior-predictive accumulator of include/logreg_hip_predict.h: draws beta_s [S][P] and prediction
// rows x_i [r][P] -> per-row moments of pi = sigma(x.beta), L = sigma(t) and l = log sigma(t), t = (2y - 1) x.beta.
//
// Layout.  A lane owns a prediction row: its x_i and its five float64 accumulators live in registers.  blockIdx.x = tile of 256
// rows, blockIdx.y = slice of the draws; a workgroup walks its slice draw by draw.  The address of beta_s depends on blockIdx.y and the
// loop counter alone, so it is wave-uniform: the compiler loads the draw through the scalar unit (s_load_dwordx8 / x16) and the dot
// product's v_fma reads it as an SGPR operand -- no LDS, no cross-lane traffic, no reduction.  Rows wider than 64 registers (float32
// beyond p = 64, float64 beyond p = 32) do not stay in registers: their coordinates are re-read in chunks of 128 bytes (from L1 / L2)
// once per group of kPredGroupWide draws, whose partial logits wait in registers.
//
// Arithmetic.  Per pair, in the model's dtype T: eta by sequential fma over the coordinates; e = exp(-|t|); r = 1 / (1 + e);
// sigma(|t|) = r, sigma(-|t|) = e r; l = min(t, 0) - log1p(e) (exp_noguard / log1p_unit of lr_device.h, as row_term).  The rows are
// stored SIGNED, xs_i = (2 y_i - 1) x_i, as the model stores its own (negation is exact, so t is bit-for-bit (2y - 1) eta); pi is
// sigma(t) for y = 1 and sigma(-t) for y = 0 -- never 1 - sigma(t).  Over the draws of a slice, in float64: sums of (pi - c_pi),
// (pi - c_pi)^2, L, (l - c_l), (l - c_l)^2 with the pivots c = the values at the slice's first draw (the textbook shifted-data
// variance: the pivot is within the spread of the data, so sum d^2 - (sum d)^2 / n cancels at most a digit).  A slice ends as
// (mean, M2) partials [slices][5][r]; k_predict_merge merges them by Chan's pairwise rule over a fixed tree and folds the result
// into the running table.  No atomics: the same calls give the same bytes.
//
// A NaN coordinate in a draw reaches every lane's eta (0 * NaN = NaN as well), and no step below drops a NaN (the clamp ahead of the
// exponential is a select, not fmax; the reciprocal is pred_rcp, without fast_rcp's fmin), so every entry of the table becomes NaN.
// L <= 1: its mean needs no max-shifted log-sum-exp; L underflows only for t < -708 in float64 (include/logreg_hip_predict.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_device.h"

namespace lr {

constexpr int kPredRows = 5;
constexpr int kPredBlock = 256;      // lanes = rows per workgroup of k_predict_partial
constexpr int kPredGroup = 4;        // draws in flight per lane (independent dependency chains; rows in registers)
constexpr int kPredGroupWide = 8;    // ... when the row is re-read per group (wide rows)
constexpr int kPredMergeRows = 64;   // k_predict_merge: block = (64 rows, 16 slice ranges)
constexpr int kPredMergeWays = 16;

template <typename T, int P> struct PredGeom {
    static constexpr int DW = (int)sizeof(T) / 4;
    static constexpr int CH = P * DW <= 64 ? P : 32 / DW;  // coordinates held in registers at a time (wide rows: 128 bytes)
    static constexpr int NCH = P / CH;
    // draws in flight: their coordinates wait in SGPRs (at most 64 of them), the wide rows' partial logits in VGPRs
    static constexpr int DG = NCH > 1 ? kPredGroupWide : (kPredGroup * P * DW <= 64 ? kPredGroup : (64 / (P * DW) > 0 ? 64 / (P * DW) : 1));
};

// 1 / x for x in [1, 2] or NaN.  float64: the seed and the two Newton steps of fast_rcp WITHOUT its clamp of x = inf -- 1 + e cannot
// overflow here, and the clamp is an fmin, which answers 1e300 to a NaN: sigma(|t|) = r would come out finite for a NaN draw.  The
// same bits as fast_rcp for every finite argument.
__device__ __forceinline__ float pred_rcp(float x) { return fast_rcp(x); }
__device__ __forceinline__ double pred_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}

// pi, L, l of one pair from t (= eta where there are no labels; `pos`: y = 1 or no label).  t = NaN gives NaN in all three: e and with
// it r and e r are NaN, so whichever way the selects on t fall, they choose between NaNs.
template <typename T>
__device__ __forceinline__ void pred_pair(T t, bool pos, T& pi, T& L, T& l) {
    const T na = -__builtin_fabs(t);
    T e;
    if constexpr (sizeof(T) == 8) e = exp_noguard(na < T(-750) ? T(-750) : na);
    else e = fast_exp(na);
    const T r = pred_rcp(T(1) + e), er = e * r;
    const bool nonneg = t >= T(0);
    L = nonneg ? r : er;
    const T Lc = nonneg ? er : r;
    pi = pos ? L : Lc;
    l = (t < T(0) ? t : T(0)) - log1p_unit(e);
}

struct PredSums {  // float64 sums over the draws of a slice, shifted by the pivots
    double c_pi, c_l, s_pi, q_pi, s_L, s_l, q_l;
};

template <typename T, bool LABELS>
__device__ __forceinline__ void pred_fold(PredSums& a, T t, bool pos) {
    T pi, L, l;
    pred_pair<T>(t, pos, pi, L, l);
    const double d = (double)pi - a.c_pi;
    a.s_pi += d;
    a.q_pi = __builtin_fma(d, d, a.q_pi);
    if constexpr (LABELS) {
        const double dl = (double)l - a.c_l;
        a.s_L += (double)L;
        a.s_l += dl;
        a.q_l = __builtin_fma(dl, dl, a.q_l);
    }
}

// logits of DG consecutive draws (b: wave-uniform, [DG][P]) against this lane's row
template <typename T, int P, int DG>
__device__ __forceinline__ void pred_eta(const T* __restrict__ xrow, const T (&x)[PredGeom<T, P>::CH], const T* __restrict__ b, T (&eta)[DG]) {
    constexpr int CH = PredGeom<T, P>::CH, NCH = PredGeom<T, P>::NCH;
#pragma unroll
    for (int d = 0; d < DG; ++d) eta[d] = T(0);
    if constexpr (NCH == 1) {
#pragma unroll
        for (int d = 0; d < DG; ++d)
#pragma unroll
            for (int j = 0; j < CH; ++j) eta[d] = fma_t(x[j], b[d * P + j], eta[d]);
    } else {
#pragma unroll 1
        for (int c = 0; c < NCH; ++c) {
            int off = c * CH;
            asm volatile("" : "+v"(off));  // the chunk is re-read here on every trip: hoisted out of the draw loop, the whole row would want registers
            T xc[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) xc[j] = xrow[off + j];
#pragma unroll
            for (int d = 0; d < DG; ++d) {
#pragma unroll
                for (int j = 0; j < CH; ++j) eta[d] = fma_t(xc[j], b[d * P + c * CH + j], eta[d]);
                // one draw's 128 bytes of coordinates in SGPRs at a time: left alone, the scheduler starts the loads of all DG draws at
                // once and the 256 SGPRs they want go through v_writelane / v_readlane (1.2 such moves per fma); other waves hide the load
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// rows [r][P] signed rows; sign [r]: +1 / -1 (read only with LABELS); draws [S][P]; slice y takes draws [y per, min(S, (y + 1) per));
// part [gridDim.y][kPredRows][r].  Every slice is non-empty by construction (the host derives the slice count from per).
template <typename T, int P, bool LABELS>
__global__ void __launch_bounds__(kPredBlock) k_predict_partial(const T* __restrict__ rows, const signed char* __restrict__ sign, int64_t r,
                                                                const T* __restrict__ draws, int64_t S, int64_t per, double* __restrict__ part) {
    constexpr int CH = PredGeom<T, P>::CH, NCH = PredGeom<T, P>::NCH, DG = PredGeom<T, P>::DG;
    const int64_t i = (int64_t)blockIdx.x * kPredBlock + threadIdx.x;
    const int64_t il = i < r ? i : r - 1;  // lanes past the last row redo it and store nothing
    const T* __restrict__ xrow = rows + il * P;
    T x[CH];
    if constexpr (NCH == 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) x[j] = xrow[j];
    }
    bool pos = true;
    if constexpr (LABELS) pos = sign[il] > 0;
    const int64_t s0 = (int64_t)blockIdx.y * per, s1 = s0 + per < S ? s0 + per : S;

    PredSums a{};
    {  // the slice's first draw gives the pivots
        T eta[1];
        pred_eta<T, P, 1>(xrow, x, draws + s0 * P, eta);
        T pi, L, l;
        pred_pair<T>(eta[0], pos, pi, L, l);
        a.c_pi = (double)pi;
        a.c_l = (double)l;
        a.s_L = (double)L;
    }
    int64_t s = s0 + 1;
    for (; s + DG <= s1; s += DG) {
        T eta[DG];
        pred_eta<T, P, DG>(xrow, x, draws + s * P, eta);
#pragma unroll
        for (int d = 0; d < DG; ++d) pred_fold<T, LABELS>(a, eta[d], pos);
    }
    for (; s < s1; ++s) {
        T eta[1];
        pred_eta<T, P, 1>(xrow, x, draws + s * P, eta);
        pred_fold<T, LABELS>(a, eta[0], pos);
    }
    if (i < r) {
        const double n = (double)(s1 - s0), inv = 1.0 / n;
        double* __restrict__ o = part + (int64_t)blockIdx.y * kPredRows * r + i;
        o[0] = __builtin_fma(a.s_pi, inv, a.c_pi);
        o[r] = __builtin_fma(-a.s_pi * inv, a.s_pi, a.q_pi);
        o[2 * r] = a.s_L * inv;
        o[3 * r] = __builtin_fma(a.s_l, inv, a.c_l);
        o[4 * r] = __builtin_fma(-a.s_l * inv, a.s_l, a.q_l);
    }
}

// src [S][p] -> dst [S][P], zero in the padded coordinates (draws of a model whose p is not one of the padded widths)
template <typename T>
__global__ void __launch_bounds__(256) k_predict_pad(const T* __restrict__ src, int64_t S, int p, int P, T* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= S * P) return;
    const int64_t s = e / P;
    const int j = (int)(e - s * P);
    dst[e] = j < p ? src[s * p + j] : T(0);
}

struct PredMoments {  // (count, mean pi, M2 pi, mean L, mean l, M2 l) of a set of draws; merge = Chan, Golub & LeVeque, every product spelled as fma
    double n, m_pi, q_pi, m_L, m_l, q_l;
    __device__ __forceinline__ void merge(const PredMoments& b) {
        if (b.n <= 0.0) return;
        if (n <= 0.0) { *this = b; return; }
        const double tot = n + b.n, w = b.n / tot, nw = n * w;
        const double d = b.m_pi - m_pi, dl = b.m_l - m_l;
        m_pi = __builtin_fma(d, w, m_pi);
        q_pi = __builtin_fma(d * d, nw, q_pi + b.q_pi);
        m_L = __builtin_fma(b.m_L - m_L, w, m_L);
        m_l = __builtin_fma(dl, w, m_l);
        q_l = __builtin_fma(dl * dl, nw, q_l + b.q_l);
        n = tot;
    }
};

// block = (kPredMergeRows, kPredMergeWays): thread (x, y) merges the slices of range y in slice order, the ranges are merged by a
// fixed binary tree, and the result is folded into the running table acc [kPredRows][r] that holds n0 draws (n0 = 0: acc is not read).
__global__ void __launch_bounds__(kPredMergeRows* kPredMergeWays) k_predict_merge(const double* __restrict__ part, int64_t slices, int64_t per,
                                                                                   int64_t S, int64_t r, double n0, double* __restrict__ acc) {
    __shared__ PredMoments red[kPredMergeWays][kPredMergeRows];
    const int64_t i = (int64_t)blockIdx.x * kPredMergeRows + threadIdx.x;
    const int y = threadIdx.y;
    const int64_t chunk = (slices + kPredMergeWays - 1) / kPredMergeWays;
    const int64_t k0 = y * chunk, k1 = k0 + chunk < slices ? k0 + chunk : slices;
    PredMoments m{0, 0, 0, 0, 0, 0};
    if (i < r) {
        for (int64_t k = k0; k < k1; ++k) {
            const double* q = part + k * kPredRows * r + i;
            const int64_t cnt = (k + 1) * per <= S ? per : S - k * per;
            m.merge(PredMoments{(double)cnt, q[0], q[r], q[2 * r], q[3 * r], q[4 * r]});
        }
    }
    red[y][threadIdx.x] = m;
    __syncthreads();
    for (int half = kPredMergeWays / 2; half >= 1; half >>= 1) {
        if (y < half) {
            PredMoments a = red[y][threadIdx.x];
            a.merge(red[y + half][threadIdx.x]);
            red[y][threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (y == 0 && i < r) {
        PredMoments t{0, 0, 0, 0, 0, 0};
        if (n0 > 0.0) t = PredMoments{n0, acc[i], acc[r + i], acc[2 * r + i], acc[3 * r + i], acc[4 * r + i]};
        t.merge(red[0][threadIdx.x]);
        acc[i] = t.m_pi;
        acc[r + i] = t.q_pi;
        acc[2 * r + i] = t.m_L;
        acc[3 * r + i] = t.m_l;
        acc[4 * r + i] = t.q_l;
    }
}

}  // namespace lr
