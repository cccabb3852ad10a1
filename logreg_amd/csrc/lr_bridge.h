// lr_bridge.h -- bridge sampling of include/logreg_hip_bridge.h: draws theta_s [S][P] -> the float64 terms l_s = lpost(theta_s) - log g(theta_s)
// (k_bridge_fill, k_bridge_gauss), the proposal draws mu + L z (k_bridge_propose), and the iteration with its error over the stored
// terms (k_bridge_iterate, k_bridge_finish).
//
// k_bridge_fill.  k_predict_partial's layout: a lane owns a row (x_i in registers, the draws arriving through the scalar unit: pred_eta /
// pred_pair of lr_predict.h, unchanged), but where that kernel sums over the draws of a slice, this one sums over the ROWS, per draw.
// blockIdx.x = slice of kBridgeSliceRows rows, blockIdx.y = slice of the draws.  A workgroup takes DG draws at a time (the draws in flight
// of PredGeom): a lane adds the row terms of its rows t, t + 256 into DG float64 partial sums, the wave reduces each by the fixed
// butterfly of group_sum<64> (DPP inside a 16-lane row, v_permlane swaps across rows: both partners form the same sum), the four waves'
// sums meet in LDS and are added in wave order.  part [row slices][ld]: k_bridge_gauss adds the slices in slice order.  A draw's sum
// involves no other draw and no launch parameter but n, so its bytes do not depend on how the draws were cut into calls, pieces,
// chunks or draw slices.  The row is re-read (from L1 / L2) once per DG draws: with two row tiles a slice the butterfly, 30 instructions
// a draw and wave, is paid once per 128 row terms.
//
// k_bridge_gauss.  A lane owns a draw; a workgroup is one wave.  d = theta - mu goes to LDS transposed, dT [P][64], so that lane t reads
// dT[j][t]: consecutive lanes on consecutive addresses, and no array indexed at run time lives in registers.  W = L^-1 (packed lower
// triangle) and mu are read at wave-uniform addresses.  The same kernel adds the row slices and the prior: one launch per chunk
// finishes the terms.  k_bridge_propose has the same shape with z in place of d and L in place of W.
//
// k_bridge_iterate + k_bridge_finish.  One pass over the stored terms per launch, blocks of kBridgeChunk terms, and a single-workgroup
// launch that adds the blocks' partials and updates the state; the HOST loops, reading log r (two doubles) per iteration.  The
// alternative, one launch with the loop inside, must run on one workgroup (or pay a grid barrier per pass): 2^21 logaddexp per pass on one
// CU against all of them, for three or four round trips of a few tens of microseconds saved.  Float64 throughout, products inside
// sums spelled fma, no atomics: lane t adds its terms t, t + 256, ... in order, butterfly, waves in order -- a fixed tree for (N1, N2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "lr_loo.h"
#include "lr_predict.h"

namespace lr {

constexpr int kBridgeRows = 12;
constexpr int64_t kBridgeMaxDraws = 1 << 20;
constexpr uint32_t TAG_BRIDGE = 0x08000000u;  // | b: normal block b of a proposal draw (LR_BRIDGE_TAG)
constexpr int kBridgeBlock = 256;             // lanes of k_bridge_fill, k_bridge_iterate, k_bridge_finish
constexpr int kBridgeRowTiles = 2;            // rows per lane and slice
constexpr int kBridgeSliceRows = kBridgeBlock * kBridgeRowTiles;
constexpr int kBridgeGaussBlock = 64;         // draws per workgroup of k_bridge_gauss / k_bridge_propose
constexpr int kBridgeChunk = 4096;            // terms per workgroup of k_bridge_iterate
constexpr int kBridgeMaxP = 128;
enum { BR_SCAN = 0, BR_INIT = 1, BR_ITER = 2, BR_ERR = 3 };
// the state of a solve, device doubles
enum { BS_LOGR = 0, BS_PREV = 1, BS_MIN1 = 2, BS_MAX1 = 3, BS_MIN2 = 4, BS_MAX2 = 5, BS_BAD = 6, BS_RE2 = 7, BS_SLOTS = 8 };

// ---- the proposal's factor (host, float64, nothing contracted): L and W = L^-1 as packed lower triangles [p (p + 1) / 2] (entry (i, j) at
// i (i + 1) / 2 + j), c_g = -sum log L_ii - p / 2 log(2 pi).  -> 0, or -1 with the reason in `why`.
inline int bridge_factor(int p, const double* mu, const double* cov, double* L_out, double* W_out, double* cg_out, char* why, size_t why_len) {
#pragma clang fp contract(off)
    if (p < 1 || p > kBridgeMaxP) {
        std::snprintf(why, why_len, "p must be in 1..%d (got %d)", kBridgeMaxP, p);
        return -1;
    }
    for (int i = 0; i < p; ++i) {
        if (!std::isfinite(mu[i])) {
            std::snprintf(why, why_len, "mu[%d] is not finite", i);
            return -1;
        }
        for (int j = 0; j <= i; ++j)
            if (!std::isfinite(cov[i * p + j])) {
                std::snprintf(why, why_len, "cov[%d][%d] is not finite", i, j);
                return -1;
            }
    }
    std::vector<double> L((size_t)p * p, 0.0), W((size_t)p * p, 0.0);
    double logdet = 0.0;
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            double t = cov[i * p + j];
            for (int k = 0; k < j; ++k) {
                const double q = L[i * p + k] * L[j * p + k];
                t = t - q;
            }
            if (i == j) {
                if (!(t > 0) || !std::isfinite(t)) {
                    std::snprintf(why, why_len, "cov is not positive definite: pivot %d is %g", i, t);
                    return -1;
                }
                L[i * p + i] = std::sqrt(t);
                logdet = logdet + std::log(L[i * p + i]);
            } else {
                L[i * p + j] = t / L[j * p + j];
            }
        }
    for (int c = 0; c < p; ++c)  // column c of W: L W = I by forward substitution
        for (int i = c; i < p; ++i) {
            double t = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) {
                const double q = L[i * p + k] * W[k * p + c];
                t = t - q;
            }
            W[i * p + c] = t / L[i * p + i];
        }
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            L_out[i * (i + 1) / 2 + j] = L[i * p + j];
            W_out[i * (i + 1) / 2 + j] = W[i * p + j];
        }
    *cg_out = -logdet - 0.5 * p * 1.8378770664093453;  // log(2 pi)
    return 0;
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------------
// DT consecutive draws (b: wave-uniform, [DT][P]) against the rows of slice row0: out[d] = the slice's row sum for draw d.  red: 4 DT slots
// of LDS, free on entry (two barriers inside).  Every lane of the workgroup is active.
template <typename T, int P, int DT>
__device__ __forceinline__ void bridge_tile(const T* __restrict__ rows, int64_t n, int64_t row0, const T* __restrict__ b, double* red, double* __restrict__ out) {
    constexpr int CH = PredGeom<T, P>::CH, NCH = PredGeom<T, P>::NCH;
    const int tid = threadIdx.x;
    double acc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) acc[d] = 0.0;
#pragma unroll 1
    for (int t = 0; t < kBridgeRowTiles; ++t) {
        const int64_t base = row0 + (int64_t)t * kBridgeBlock;
        if (base >= n) break;  // (the same for every lane)
        const int64_t i = base + tid, il = i < n ? i : n - 1;  // lanes past the last row redo it and add 0
        const T* __restrict__ xrow = rows + il * P;
        T x[CH];
        if constexpr (NCH == 1) {
#pragma unroll
            for (int j = 0; j < CH; ++j) x[j] = xrow[j];
        }
        T eta[DT];
        pred_eta<T, P, DT>(xrow, x, b, eta);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            T pi, L, l;
            pred_pair<T>(eta[d], true, pi, L, l);
            acc[d] += i < n ? (double)l : 0.0;
        }
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) acc[d] = group_sum<64>(acc[d]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int d = 0; d < DT; ++d) red[(tid >> 6) * DT + d] = acc[d];
    }
    __syncthreads();
    if (tid < DT) out[tid] = ((red[tid] + red[DT + tid]) + red[2 * DT + tid]) + red[3 * DT + tid];
    __syncthreads();
}

// rows [n][P] signed rows; draws [S][P]; draw slice y takes draws [y per, min(S, (y + 1) per)); part [gridDim.x][ld], ld >= S: the sum
// of row slice x for draw s at part[x ld + s].
template <typename T, int P>
__global__ void __launch_bounds__(kBridgeBlock) k_bridge_fill(const T* __restrict__ rows, int64_t n, const T* __restrict__ draws, int64_t S, int64_t per,
                                                              double* __restrict__ part, int64_t ld) {
    constexpr int DG = PredGeom<T, P>::DG;
    __shared__ double red[4 * DG];
    const int64_t row0 = (int64_t)blockIdx.x * kBridgeSliceRows;
    const int64_t s0 = (int64_t)blockIdx.y * per, s1 = s0 + per < S ? s0 + per : S;
    double* __restrict__ o = part + (int64_t)blockIdx.x * ld;
    int64_t s = s0;
    for (; s + DG <= s1; s += DG) bridge_tile<T, P, DG>(rows, n, row0, draws + s * P, red, o + s);
    for (; s < s1; ++s) bridge_tile<T, P, 1>(rows, n, row0, draws + s * P, red, o + s);
}

// ---- the Gaussian, the prior and the merge of the row slices -----------------------------------------------------------------------------
// prop: mu [p] | inv_var [p] | W packed [p (p + 1) / 2] | L packed (not read here).  l_out[s] = (sum of the slices + lprior) - log g.
template <typename T, int P>
__global__ void __launch_bounds__(kBridgeGaussBlock) k_bridge_gauss(const T* __restrict__ draws, int64_t S, int p, const double* __restrict__ part, int64_t ld,
                                                                    int64_t rslices, const double* __restrict__ prop, double cg, double lprior_const,
                                                                    double* __restrict__ l_out) {
#pragma clang fp contract(off)
    __shared__ double dT[P][kBridgeGaussBlock];
    const int lane = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * kBridgeGaussBlock + lane, sl = s < S ? s : S - 1;
    const T* __restrict__ th = draws + sl * P;
    const double* __restrict__ mu = prop;
    const double* __restrict__ inv_var = prop + p;
    const double* __restrict__ Wrow = prop + 2 * p;
    double pr = 0.0;
    for (int j = 0; j < p; ++j) {
        const double t = (double)th[j];
        pr = __builtin_fma(inv_var[j] * t, t, pr);
        dT[j][lane] = t - mu[j];  // (read back by this lane alone)
    }
    double q = 0.0;
    for (int i = 0; i < p; ++i) {
        double y = 0.0;
        for (int j = 0; j <= i; ++j) y = __builtin_fma(Wrow[j], dT[j][lane], y);
        q = __builtin_fma(y, y, q);
        Wrow += i + 1;
    }
    double ll = part[sl];
    for (int64_t k = 1; k < rslices; ++k) ll += part[k * ld + sl];
    const double lpost = ll + __builtin_fma(-0.5, pr, lprior_const);
    if (s < S) l_out[s] = lpost - __builtin_fma(-0.5, q, cg);
}

// out [cnt][ldo], ldo = P (zero in the padded coordinates) or p: draw j0 + k = mu + L z_k rounded to T
template <typename T, int P>
__global__ void __launch_bounds__(kBridgeGaussBlock) k_bridge_propose(uint64_t seed, int64_t j0, int64_t cnt, int p, int ldo,
                                                                      const double* __restrict__ prop, T* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double zT[P][kBridgeGaussBlock];
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * kBridgeGaussBlock + lane;
    const uint64_t j = (uint64_t)(j0 + (k < cnt ? k : cnt - 1));
    for (int b = 0; 4 * b < p; ++b) {  // (P is a multiple of 4: the block's four normals all have a slot)
        const U4 w = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 0u, TAG_BRIDGE | (uint32_t)b, (uint32_t)seed, (uint32_t)(seed >> 32));
        T a0, a1, a2, a3;
        box_muller(w.x, w.y, a0, a1);
        box_muller(w.z, w.w, a2, a3);
        zT[4 * b + 0][lane] = (double)a0;
        zT[4 * b + 1][lane] = (double)a1;
        zT[4 * b + 2][lane] = (double)a2;
        zT[4 * b + 3][lane] = (double)a3;
    }
    if (k >= cnt) return;
    const double* __restrict__ mu = prop;
    const double* __restrict__ Lrow = prop + 2 * p + p * (p + 1) / 2;
    T* __restrict__ o = out + k * ldo;
    for (int i = 0; i < p; ++i) {
        double t = mu[i];
        for (int c = 0; c <= i; ++c) t = __builtin_fma(Lrow[c], zT[c][lane], t);
        o[i] = (T)t;
        Lrow += i + 1;
    }
    for (int i = p; i < ldo; ++i) o[i] = T(0);
}

// ---- the iteration -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bridge_lae(double x, double y) {  // logaddexp of two finite numbers
    const double m = x > y ? x : y;
    return m + log1p(exp(-__builtin_fabs(x - y)));
}
// the largest term of each log-sum-exp of an iteration: both are monotone in l
__device__ __forceinline__ double bridge_top2(double max2, double lr, double ls1, double ls2) { return max2 - bridge_lae(ls1 + max2, ls2 + lr); }
__device__ __forceinline__ double bridge_top1(double min1, double lr, double ls1, double ls2) { return -bridge_lae(ls1 + min1, ls2 + lr); }
// the two quotients of the error: p / (s1 p + s2 g) at a proposal term (written so that an overflowing exp gives 0), g / (s1 p + s2 g) at a posterior term
__device__ __forceinline__ double bridge_f1(double l2, double lr, double s1, double s2) { return 1.0 / __builtin_fma(s2, exp(lr - l2), s1); }
__device__ __forceinline__ double bridge_f2(double l1, double lr, double s1, double s2) { return 1.0 / __builtin_fma(s1, exp(l1 - lr), s2); }

// One pass.  Workgroup b < nb2 takes terms [b, b + 1) kBridgeChunk of l2, workgroup nb2 + b those of l1 (BR_INIT: l2 alone, nb2 workgroups).
// part [gridDim.x][3]:  BR_SCAN  min, max over the finite terms, the count of the others
//                       BR_INIT  sum exp(l2 - max l2)                      BR_ITER  sum exp(term - largest term)
//                       BR_ERR   sum d, sum d^2 of d = f - pivot
__global__ void __launch_bounds__(kBridgeBlock) k_bridge_iterate(int mode, const double* __restrict__ l1, int64_t N1, const double* __restrict__ l2, int64_t N2,
                                                                 int64_t nb2, double ls1, double ls2, double s1, double s2, const double* __restrict__ st,
                                                                 double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double buf[kBridgeBlock / 64];
    const bool two = (int64_t)blockIdx.x < nb2;
    const double* __restrict__ v = two ? l2 : l1;
    const int64_t N = two ? N2 : N1, b = two ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - nb2;
    const int64_t e0 = b * kBridgeChunk, e1 = e0 + kBridgeChunk < N ? e0 + kBridgeChunk : N;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (mode == BR_SCAN) {
        double mn = __builtin_inf(), mx = -__builtin_inf(), bad = 0.0;
        for (int64_t e = e0 + threadIdx.x; e < e1; e += kBridgeBlock) {
            const double x = v[e];
            const bool fin = __builtin_fabs(x) < __builtin_inf();  // false for NaN
            mn = fin && x < mn ? x : mn;
            mx = fin && x > mx ? x : mx;
            bad += fin ? 0.0 : 1.0;
        }
        a0 = loo_block_red<kBridgeBlock>(mn, [](double x, double y) { return x < y ? x : y; }, buf);
        a1 = loo_block_red<kBridgeBlock>(mx, [](double x, double y) { return x > y ? x : y; }, buf);
        a2 = loo_block_sum<kBridgeBlock>(bad, buf);
    } else {
        const double lr = st[BS_LOGR], min1 = st[BS_MIN1], max2 = st[BS_MAX2];
        double sa = 0.0, sb = 0.0;
        if (mode == BR_INIT) {
            for (int64_t e = e0 + threadIdx.x; e < e1; e += kBridgeBlock) sa += exp(v[e] - max2);
        } else if (mode == BR_ITER) {
            const double top = two ? bridge_top2(max2, lr, ls1, ls2) : bridge_top1(min1, lr, ls1, ls2), c = ls2 + lr;
            for (int64_t e = e0 + threadIdx.x; e < e1; e += kBridgeBlock) {
                const double x = v[e], lae = bridge_lae(ls1 + x, c);
                sa += exp((two ? x - lae : -lae) - top);
            }
        } else {
            const double c = two ? bridge_f1(max2, lr, s1, s2) : bridge_f2(min1, lr, s1, s2);
            for (int64_t e = e0 + threadIdx.x; e < e1; e += kBridgeBlock) {
                const double x = v[e], d = (two ? bridge_f1(x, lr, s1, s2) : bridge_f2(x, lr, s1, s2)) - c;
                sa += d;
                sb = __builtin_fma(d, d, sb);
            }
        }
        a0 = loo_block_sum<kBridgeBlock>(sa, buf);
        a1 = loo_block_sum<kBridgeBlock>(sb, buf);
    }
    if (threadIdx.x == 0) {
        double* __restrict__ o = part + (int64_t)blockIdx.x * 3;
        o[0] = a0;
        o[1] = a1;
        o[2] = a2;
    }
}

// column c of the partials [first, first + count) combined: lane t takes partials t, t + 256, ... in order, butterfly, waves in order
template <typename F>
__device__ __forceinline__ double bridge_fold(const double* __restrict__ part, int64_t first, int64_t count, int c, double unit, F f, double* buf) {
    double a = unit;
    for (int64_t b = threadIdx.x; b < count; b += kBridgeBlock) a = f(a, part[(first + b) * 3 + c]);
    return loo_block_red<kBridgeBlock>(a, f, buf);
}

// A single workgroup: the partials of a pass -> the state.  n1, n2, neff: N1, N2 and the effective size as doubles.
__global__ void __launch_bounds__(kBridgeBlock) k_bridge_finish(int mode, const double* __restrict__ part, int64_t nb1, int64_t nb2, double n1, double n2,
                                                                double neff, double ls1, double ls2, double s1, double s2, double* __restrict__ st) {
#pragma clang fp contract(off)
    __shared__ double buf[kBridgeBlock / 64];
    const auto add = [](double x, double y) { return x + y; };
    const auto lo = [](double x, double y) { return x < y ? x : y; };
    const auto hi = [](double x, double y) { return x > y ? x : y; };
    const double inf = __builtin_inf();
    if (mode == BR_SCAN) {
        const double mn2 = bridge_fold(part, 0, nb2, 0, inf, lo, buf), mx2 = bridge_fold(part, 0, nb2, 1, -inf, hi, buf);
        const double mn1 = bridge_fold(part, nb2, nb1, 0, inf, lo, buf), mx1 = bridge_fold(part, nb2, nb1, 1, -inf, hi, buf);
        const double bad = bridge_fold(part, 0, nb2, 2, 0.0, add, buf) + bridge_fold(part, nb2, nb1, 2, 0.0, add, buf);
        if (threadIdx.x == 0) {
            const double nan = __builtin_nan("");
            st[BS_MIN1] = mn1 <= mx1 ? mn1 : nan;  // (no finite term: NaN)
            st[BS_MAX1] = mn1 <= mx1 ? mx1 : nan;
            st[BS_MIN2] = mn2 <= mx2 ? mn2 : nan;
            st[BS_MAX2] = mn2 <= mx2 ? mx2 : nan;
            st[BS_BAD] = bad;
            st[BS_LOGR] = st[BS_PREV] = st[BS_RE2] = nan;
        }
    } else if (mode == BR_INIT) {
        const double sum2 = bridge_fold(part, 0, nb2, 0, 0.0, add, buf);
        if (threadIdx.x == 0) st[BS_LOGR] = st[BS_MAX2] + (log(sum2) - log(n2));
    } else if (mode == BR_ITER) {
        const double sum2 = bridge_fold(part, 0, nb2, 0, 0.0, add, buf), sum1 = bridge_fold(part, nb2, nb1, 0, 0.0, add, buf);
        if (threadIdx.x == 0) {
            const double lr = st[BS_LOGR], c = ls2 + lr, max2 = st[BS_MAX2], min1 = st[BS_MIN1];
            // top2 - top1 with the two logaddexp side by side: equal terms cancel exactly
            const double tops = max2 + (bridge_lae(ls1 + min1, c) - bridge_lae(ls1 + max2, c));
            st[BS_PREV] = lr;
            st[BS_LOGR] = tops + ((log(sum2) - log(n2)) - (log(sum1) - log(n1)));
        }
    } else {
        const double d2 = bridge_fold(part, 0, nb2, 0, 0.0, add, buf), q2 = bridge_fold(part, 0, nb2, 1, 0.0, add, buf);
        const double d1 = bridge_fold(part, nb2, nb1, 0, 0.0, add, buf), q1 = bridge_fold(part, nb2, nb1, 1, 0.0, add, buf);
        if (threadIdx.x == 0) {
            const double lr = st[BS_LOGR];
            const double m2 = bridge_f1(st[BS_MAX2], lr, s1, s2) + d2 / n2, m1 = bridge_f2(st[BS_MIN1], lr, s1, s2) + d1 / n1;
            const double v2 = n2 > 1.0 ? __builtin_fma(-d2 / n2, d2, q2) / (n2 - 1.0) : 0.0;
            const double v1 = n1 > 1.0 ? __builtin_fma(-d1 / n1, d1, q1) / (n1 - 1.0) : 0.0;
            st[BS_RE2] = v2 / (m2 * m2 * n2) + v1 / (m1 * m1 * neff);
        }
    }
}

}  // namespace lr
