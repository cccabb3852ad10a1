// lr_ppc.h -- the posterior predictive check of include/logreg_hip_ppc.h: draws beta_s [S][P] and check rows x_i [r][P] -> per draw the
// replicated outcomes y_rep(s,i) = [u < sigma(x_i . beta_s)], their counts T_g per group of rows, and the deviances D_obs and D_rep.
//
// Layout.  k_ppc_partial is k_predict_partial's layout (lr_predict.h: a lane owns a row, x in registers or re-read in chunks, the draw
// addressed from block and loop indices alone and so loaded through the scalar unit) with a replicate and a reduction over the rows
// added.  blockIdx.x = tile of 256 rows, blockIdx.y = slice of the draws of a sub-batch.  Draws are worked off in QUADS s = 4 q .. 4 q + 3
// of the global draw index: one Philox block (counter (q lo, q hi, i, TAG_PPC)) gives the lane its four uniforms, four logits are in
// flight.  Slices start at multiples of 4 of the global index; a quad that straddles the first or last draw of the sub-batch (a call
// that starts at s mod 4 != 0) takes its draws one by one, each still with word s & 3 of the same block.
// Per draw and tile: the group counts by ballot + popcount per group (wave-uniform; lane g keeps group g's), the two deviance sums by
// the DPP / permlane butterfly of group_sum<64> in float64; the four waves meet in LDS ((w0 + w1) + (w2 + w3), two buffers, one
// barrier per quad).  Out: partials [tile][draw] and, per lane, the count of ones over the slice, added to row_ones by one 64-bit integer
// atomic.  k_ppc_fold sums the tiles of a draw in ascending order, bumps hist / dev_ge / n_nonfinite with 64-bit integer atomics and
// leaves (D_obs, D_rep); k_ppc_moments merges those into the running moments over a fixed tree.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_device.h"
#include "lr_predict.h"

namespace lr {

constexpr uint32_t TAG_PPC = 0x04000000u;
constexpr int kPpcBlock = kPredBlock;  // lanes = rows per workgroup
constexpr int kPpcWaves = kPpcBlock / 64;
constexpr int kPpcMaxGroups = 32;
constexpr int kPpcMomBlock = 256;
constexpr int kPpcState = 5;  // the running moments: finite draws, mean and M2 of D_obs, mean and M2 of D_rep

// pi = sigma(eta), l_y = log sigma(t) and l_o = log sigma(-t) from the signed logit t = (2 y - 1) eta (`pos`: y = 1, or no label): the
// arithmetic of pred_pair, one exponential and one log1p for the three.  t = NaN gives NaN in all three.
template <typename T>
__device__ __forceinline__ void ppc_pair(T t, bool pos, T& pi, T& l_y, T& l_o) {
    const T na = -__builtin_fabs(t);
    T e;
    if constexpr (sizeof(T) == 8) e = exp_noguard(na < T(-750) ? T(-750) : na);
    else e = fast_exp(na);
    const T r = pred_rcp(T(1) + e), er = e * r;
    const bool nonneg = t >= T(0);
    const T L = nonneg ? r : er, Lc = nonneg ? er : r;
    pi = pos ? L : Lc;
    const T lp = log1p_unit(e);
    l_y = (t < T(0) ? t : T(0)) - lp;
    l_o = (t > T(0) ? -t : T(0)) - lp;
}

// the logits of the four draws of a quad (b: wave-uniform, [4][P]), in the sub-groups k_predict_partial keeps in flight for this width
template <typename T, int P>
__device__ __forceinline__ void ppc_eta4(const T* __restrict__ xrow, const T (&x)[PredGeom<T, P>::CH], const T* __restrict__ b, T (&eta)[4]) {
    constexpr int DG = PredGeom<T, P>::NCH > 1 ? 4 : (PredGeom<T, P>::DG >= 4 ? 4 : PredGeom<T, P>::DG);
    static_assert(DG == 1 || DG == 2 || DG == 4, "a quad is a whole number of sub-groups");
#pragma unroll
    for (int k = 0; k < 4; k += DG) {
        T part[DG];
        pred_eta<T, P, DG>(xrow, x, b + k * P, part);
#pragma unroll
        for (int d = 0; d < DG; ++d) eta[k + d] = part[d];
    }
}

// flags[j] = 1 where every coordinate of draw j is finite, else 0 (bit test: no arithmetic on the coordinates)
template <typename T>
__global__ void __launch_bounds__(256) k_ppc_flag(const T* __restrict__ draws, int64_t S, int P, uint32_t* __restrict__ flags) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    bool fin = true;
    for (int c = 0; c < P; ++c) {
        if constexpr (sizeof(T) == 4) fin = fin && (__builtin_bit_cast(uint32_t, draws[j * P + c]) & 0x7F800000u) != 0x7F800000u;
        else fin = fin && (__builtin_bit_cast(uint64_t, draws[j * P + c]) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
    }
    flags[j] = fin ? 1u : 0u;
}

// rows [r][P] signed rows; sign [r] +1 / -1 (read only with LABELS); grp [r] group labels (read only with G > 1).  The sub-batch holds
// the draws of global index [s_begin, s_end) at draws [nb][P] with flags [nb], nb = s_end - s_begin; slice y takes the global indices
// [base + y per, base + (y + 1) per) of them, base = s_begin rounded down to a multiple of 4, per a multiple of 4.
// part_d [tiles][nb][2] (D_obs, D_rep of the tile), part_c [tiles][nb][G]; row_ones [r] or NULL; yrep [nb][words] or NULL.
template <typename T, int P, bool LABELS>
__global__ void __launch_bounds__(kPpcBlock) k_ppc_partial(const T* __restrict__ rows, const signed char* __restrict__ sign, const unsigned char* __restrict__ grp,
                                                           int64_t r, int G, const T* __restrict__ draws, const uint32_t* __restrict__ flags, int64_t s_begin,
                                                           int64_t s_end, int64_t per, uint32_t seed_lo, uint32_t seed_hi, double* __restrict__ part_d,
                                                           uint32_t* __restrict__ part_c, unsigned long long* __restrict__ row_ones, uint32_t* __restrict__ yrep,
                                                           int64_t words) {
    constexpr int CH = PredGeom<T, P>::CH, NCH = PredGeom<T, P>::NCH;
    __shared__ double sh_d[2][kPpcWaves][4][2];
    __shared__ uint32_t sh_c[2][kPpcWaves][4][kPpcMaxGroups];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kPpcBlock + threadIdx.x;
    const bool valid = i < r;
    const int64_t il = valid ? i : r - 1;  // lanes past the last row redo it and count for nothing
    const T* __restrict__ xrow = rows + il * P;
    T x[CH];
    if constexpr (NCH == 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) x[j] = xrow[j];
    }
    bool pos = true;
    if constexpr (LABELS) pos = sign[il] > 0;
    int g_i = 0;
    if (G > 1) g_i = grp[il];
    const int64_t nb = s_end - s_begin, base = s_begin & ~(int64_t)3;
    const int64_t a0 = base + (int64_t)blockIdx.y * per, a1 = a0 + per < s_end ? a0 + per : s_end;
    uint32_t ones = 0;
    int par = 0;
    for (int64_t q0 = a0; q0 < a1; q0 += 4, par ^= 1) {
        const uint64_t q = (uint64_t)q0 >> 2;
        const U4 w4 = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)il, TAG_PPC, seed_lo, seed_hi);
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
        T eta[4];
        if (q0 >= s_begin && q0 + 4 <= s_end) {
            ppc_eta4<T, P>(xrow, x, draws + (q0 - s_begin) * P, eta);
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                eta[d] = T(0);
                if (q0 + d >= s_begin && q0 + d < s_end) {
                    T one[1];
                    pred_eta<T, P, 1>(xrow, x, draws + (q0 + d - s_begin) * P, one);
                    eta[d] = one[0];
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int64_t s = q0 + d;
            const bool inr = s >= s_begin && s < s_end;  // wave-uniform, as fin
            bool fin = false;
            if (inr) fin = flags[s - s_begin] != 0u;
            T pi, l_y, l_o;
            ppc_pair<T>(eta[d], pos, pi, l_y, l_o);
            const bool one = u01<T>(w[d]) < pi;  // false for a NaN pi
            const bool rep = one && valid && fin;
            const unsigned long long mask = __ballot(rep);
            ones += rep ? 1u : 0u;
            if (yrep && inr && lane == 0) {
                const int64_t w0 = (int64_t)blockIdx.x * (kPpcBlock / 32) + wave * 2;
                uint32_t* __restrict__ o = yrep + (s - s_begin) * words;
                if (w0 < words) o[w0] = (uint32_t)mask;
                if (w0 + 1 < words) o[w0 + 1] = (uint32_t)(mask >> 32);
            }
            uint32_t cnt = (uint32_t)__popcll(mask);
            for (int g = 1; g < G; ++g) {  // (group 0 last: lane 0 then holds it)
                const uint32_t c = (uint32_t)__popcll(__ballot(rep && g_i == g));
                cnt = lane == g ? c : cnt;
            }
            if (G > 1) {
                const uint32_t c = (uint32_t)__popcll(__ballot(rep && g_i == 0));
                cnt = lane == 0 ? c : cnt;
            }
            if (lane < G) sh_c[par][wave][d][lane] = cnt;
            double so = valid ? (double)l_y : 0.0;
            double sr = valid ? (double)(one == pos ? l_y : l_o) : 0.0;
            so = group_sum<64>(so);
            sr = group_sum<64>(sr);
            if (lane == 0) {
                sh_d[par][wave][d][0] = so;
                sh_d[par][wave][d][1] = sr;
            }
        }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < 8) {
            const int d = t >> 1, k = t & 1;
            const int64_t s = q0 + d;
            if (s >= s_begin && s < s_end)
                part_d[((int64_t)blockIdx.x * nb + (s - s_begin)) * 2 + k] =
                    -2.0 * ((sh_d[par][0][d][k] + sh_d[par][1][d][k]) + (sh_d[par][2][d][k] + sh_d[par][3][d][k]));
        } else if (t >= 64 && t < 64 + 4 * G) {
            const int d = (t - 64) / G, g = (t - 64) - d * G;
            const int64_t s = q0 + d;
            if (s >= s_begin && s < s_end)
                part_c[((int64_t)blockIdx.x * nb + (s - s_begin)) * G + g] = (sh_c[par][0][d][g] + sh_c[par][1][d][g]) + (sh_c[par][2][d][g] + sh_c[par][3][d][g]);
        }
    }
    if (row_ones && valid && ones) atomicAdd(row_ones + i, (unsigned long long)ones);
}

// One thread per draw j of the sub-batch: the tiles in ascending order.  With counts_out (lr_ppc_terms) it writes counts_out [nb][G] and
// dev [nb][2] and touches no table; otherwise hist[off[g] + T_g], counts[0] (D_rep >= D_obs), counts[1] (non-finite draws), dev for
// k_ppc_moments.  labels = 0: D_obs is NaN.
__global__ void __launch_bounds__(256) k_ppc_fold(const double* __restrict__ part_d, const uint32_t* __restrict__ part_c, const uint32_t* __restrict__ flags, int64_t nb,
                                                  int64_t tiles, int G, int labels, const int64_t* __restrict__ off, unsigned long long* __restrict__ hist,
                                                  unsigned long long* __restrict__ counts, double* __restrict__ dev, int32_t* __restrict__ counts_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    const bool fin = flags[j] != 0u;
    double d_obs = 0.0, d_rep = 0.0;
    for (int64_t t = 0; t < tiles; ++t) {
        d_obs += part_d[(t * nb + j) * 2];
        d_rep += part_d[(t * nb + j) * 2 + 1];
    }
    const double nan = __builtin_nan("");
    if (!labels) d_obs = nan;
    dev[j * 2] = fin ? d_obs : nan;
    dev[j * 2 + 1] = fin ? d_rep : nan;
    for (int g = 0; g < G; ++g) {
        uint32_t T = 0;
        for (int64_t t = 0; t < tiles; ++t) T += part_c[(t * nb + j) * G + g];
        if (counts_out) counts_out[j * G + g] = fin ? (int32_t)T : 0;
        else if (fin) atomicAdd(hist + off[g] + T, 1ull);
    }
    if (!counts_out) {
        if (!fin) atomicAdd(counts + 1, 1ull);
        else if (d_rep >= d_obs) atomicAdd(counts, 1ull);
    }
}

struct PpcMoments {  // (count, mean, M2) of D_obs and of D_rep over a set of draws; merge = Chan, Golub & LeVeque, products spelled as fma
    double n, m_o, q_o, m_r, q_r;
    __device__ __forceinline__ void merge(const PpcMoments& b) {
        if (b.n <= 0.0) return;
        if (n <= 0.0) { *this = b; return; }
        const double tot = n + b.n, w = b.n / tot, nw = n * w;
        const double d_o = b.m_o - m_o, d_r = b.m_r - m_r;
        m_o = __builtin_fma(d_o, w, m_o);
        q_o = __builtin_fma(d_o * d_o, nw, q_o + b.q_o);
        m_r = __builtin_fma(d_r, w, m_r);
        q_r = __builtin_fma(d_r * d_r, nw, q_r + b.q_r);
        n = tot;
    }
};

// One workgroup: thread t merges the finite draws t, t + 256, ... of dev [nb][2] in that order, the threads are merged by a fixed binary
// tree, and the result is folded into the running state [kPpcState].
__global__ void __launch_bounds__(kPpcMomBlock) k_ppc_moments(const double* __restrict__ dev, const uint32_t* __restrict__ flags, int64_t nb, double* __restrict__ state) {
    __shared__ PpcMoments red[kPpcMomBlock];
    const int t = threadIdx.x;
    PpcMoments m{0, 0, 0, 0, 0};
    for (int64_t j = t; j < nb; j += kPpcMomBlock)
        if (flags[j] != 0u) m.merge(PpcMoments{1.0, dev[j * 2], 0.0, dev[j * 2 + 1], 0.0});
    red[t] = m;
    __syncthreads();
    for (int half = kPpcMomBlock / 2; half >= 1; half >>= 1) {
        if (t < half) {
            PpcMoments a = red[t];
            a.merge(red[t + half]);
            red[t] = a;
        }
        __syncthreads();
    }
    if (t == 0) {
        PpcMoments run{state[0], state[1], state[2], state[3], state[4]};
        run.merge(red[0]);
        state[0] = run.n;
        state[1] = run.m_o;
        state[2] = run.q_o;
        state[3] = run.m_r;
        state[4] = run.q_r;
    }
}

}  // namespace lr
