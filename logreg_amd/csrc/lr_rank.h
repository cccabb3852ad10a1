// lr_rank.h -- the kernels of include/logreg_hip_rank.h: rank-normalised split-R-hat, bulk and tail ESS of stored draws X [n][C][p].
//
// Per batch of pb coordinates (grid y / z = coordinate of the batch), with h = n / 2, S = 2hC used draws and N = S rounded up to a power of
// two:
//   k_rank_gather      draw i = t C + c (time order, as stored) -> its order-preserving key (lr_rank_math.h), into U [pb][S] (kept) and into
//                      K [pb][N] (to be sorted; the N - S pads hold the largest key).
//   k_rank_sort_tile   a bitonic network on keys alone (nothing travels with a key, so stability does not matter; no atomics).  Tiles of
//   k_rank_merge_global  kRankTile keys are sorted in LDS (direction by the tile's place in the whole network); a merge of width k > tile
//                      runs its strides >= tile as one global compare-exchange launch each and finishes the strides below in LDS in one
//                      launch.  About N log2(N)^2 / 4 compare-exchanges per coordinate.
//   k_rank_quant       one thread per coordinate: med, q05, q95 (steps 3, 4) and the count of non-finite values, which sit at the two
//                      ends of the sorted keys.
//   k_rank_lookup      one thread per draw: lo / hi by two binary searches in K, 2r = lo + hi + 1 into R [pb][S], time order (what
//                      lr_rank_ranks returns).  FOLD: the key is that of f = |x - med|, recomputed from U.
//   k_rank_transform   one thread per draw: z = Phi^-1(...) of its 2r and (plain pass) the two indicators, written TRANSPOSED into
//                      V [4][pb][C][2h] (a split chain's h values are consecutive); optionally z in time order for lr_rank_ranks.
//   k_rank_fold        K <- keys of f (and pads) for the second sort.
//   k_rank_lag         one workgroup per (series, split chain): pivot at the chain's first value, the mean over a fixed tree, then thread
//                      l owns lag l: acov(l) = (1/h) sum_t e_t e_{t+l}, ONE fma per (t, l) in t order, e staged in LDS.  A [4 pb][L+2][M].
//   k_rank_partial / k_rank_final   the sums over the split chains: a fixed tree inside a workgroup of 256, the workgroups in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_rank_math.h"

namespace lr {

constexpr int kRankMaxLag = 255;
constexpr int kRankTile = 8192;        // keys per LDS tile: 64 KB
constexpr int kRankSortBlock = 1024;
constexpr int kRankLagSteps = 1024;    // time steps staged at a time
constexpr int kRankSeries = 4;         // z, zf, I05, I95
constexpr int kRankQ = 6;              // per coordinate: bits of med, q05, q95; non-finite count; keys of q05, q95

__device__ inline uint64_t rank_fold_key(uint64_t u, double med) { return lr_rank_key(__builtin_fabs(lr_rank_unkey(u) - med)); }

// number of keys < key (upper == false) or <= key (upper == true) among the sorted s[first, S)
__device__ inline int64_t rank_bound(const uint64_t* __restrict__ s, int64_t first, int64_t S, uint64_t key, bool upper) {
    int64_t lo = first, hi = S;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = s[mid];
        if (upper ? v <= key : v < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ void __launch_bounds__(256) k_rank_gather(const T* __restrict__ X, int p, int j0, int64_t S, int64_t N, uint64_t* __restrict__ U,
                                                     uint64_t* __restrict__ K) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t jb = blockIdx.y;
    if (i >= N) return;
    uint64_t key = LR_RANK_KEY_PAD;
    if (i < S) {
        key = lr_rank_key((double)X[i * p + j0 + jb]);
        U[jb * S + i] = key;
    }
    K[jb * N + i] = key;
}

__global__ void __launch_bounds__(256) k_rank_fold(const uint64_t* __restrict__ U, const uint64_t* __restrict__ Q, int64_t S, int64_t N,
                                                   uint64_t* __restrict__ K) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t jb = blockIdx.y;
    if (i >= N) return;
    const double med = __builtin_bit_cast(double, Q[jb * kRankQ]);
    K[jb * N + i] = i < S ? rank_fold_key(U[jb * S + i], med) : LR_RANK_KEY_PAD;
}

// merge == 0: the whole network on this tile (widths 2 .. tile).  merge = k > tile: the strides below a tile of the merge of width k.
__global__ void __launch_bounds__(kRankSortBlock) k_rank_sort_tile(uint64_t* __restrict__ K, int64_t N, int64_t merge) {
    __shared__ uint64_t s[kRankTile];
    const int tid = threadIdx.x;
    const int len = N < kRankTile ? (int)N : kRankTile;
    const int64_t base = (int64_t)blockIdx.x * kRankTile;
    uint64_t* g = K + (int64_t)blockIdx.y * N + base;
    for (int i = tid; i < len; i += kRankSortBlock) s[i] = g[i];
    __syncthreads();
    for (int64_t k = merge ? merge : 2; k <= (merge ? merge : (int64_t)len); k <<= 1) {
        for (int j = k > len ? len >> 1 : (int)(k >> 1); j > 0; j >>= 1) {
            for (int q = tid; q < len / 2; q += kRankSortBlock) {
                const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const int hi = lo | j;
                const bool asc = ((base + lo) & k) == 0;
                const uint64_t a = s[lo], b = s[hi];
                if ((a > b) == asc) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < len; i += kRankSortBlock) g[i] = s[i];
}

// one compare-exchange per thread: stride j >= tile of the merge of width k; N / 2 pairs
__global__ void __launch_bounds__(256) k_rank_merge_global(uint64_t* __restrict__ K, int64_t N, int64_t k, int64_t j) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= N / 2) return;
    uint64_t* g = K + (int64_t)blockIdx.y * N;
    const int64_t lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    const int64_t hi = lo | j;
    const bool asc = (lo & k) == 0;
    const uint64_t a = g[lo], b = g[hi];
    if ((a > b) == asc) {
        g[lo] = b;
        g[hi] = a;
    }
}

__global__ void __launch_bounds__(64) k_rank_quant(const uint64_t* __restrict__ K, int64_t S, int64_t N, int pb, uint64_t* __restrict__ Q) {
    const int jb = blockIdx.x * 64 + threadIdx.x;
    if (jb >= pb) return;
    const uint64_t* s = K + (int64_t)jb * N;
    const double med = (lr_rank_unkey(s[S / 2 - 1]) + lr_rank_unkey(s[S / 2])) * 0.5;
    const uint64_t k05 = s[(S - 1) / 20], k95 = s[19 * (S - 1) / 20];
    const int64_t bad = rank_bound(s, 0, S, LR_RANK_KEY_NEG_INF, true) + (S - rank_bound(s, 0, S, LR_RANK_KEY_POS_INF, false));
    uint64_t* q = Q + (int64_t)jb * kRankQ;
    q[0] = __builtin_bit_cast(uint64_t, med);
    q[1] = __builtin_bit_cast(uint64_t, lr_rank_unkey(k05));
    q[2] = __builtin_bit_cast(uint64_t, lr_rank_unkey(k95));
    q[3] = (uint64_t)bad;
    q[4] = k05;
    q[5] = k95;
}

// 2r of every draw, in time order: R [pb][S]
template <bool FOLD>
__global__ void __launch_bounds__(256) k_rank_lookup(const uint64_t* __restrict__ U, const uint64_t* __restrict__ K, const uint64_t* __restrict__ Q, int64_t S,
                                                     int64_t N, int64_t* __restrict__ R) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t jb = blockIdx.y;
    if (i >= S) return;
    const uint64_t u = U[jb * S + i];
    const uint64_t key = FOLD ? rank_fold_key(u, __builtin_bit_cast(double, Q[jb * kRankQ])) : u;
    const uint64_t* s = K + jb * N;
    const int64_t lo = rank_bound(s, 0, S, key, false);
    const int64_t hi = rank_bound(s, lo, S, key, true);
    R[jb * S + i] = lo + hi + 1;
}

// z of every draw from its 2r and (plain pass) the two indicators, transposed into V; z_out (may be NULL): z in time order, coordinate 0
template <bool FOLD>
__global__ void __launch_bounds__(256) k_rank_transform(const uint64_t* __restrict__ U, const int64_t* __restrict__ R, const uint64_t* __restrict__ Q, int64_t C,
                                                        int64_t h2, int64_t S, double* __restrict__ V, double* __restrict__ z_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t jb = blockIdx.y, pb = gridDim.y;
    if (i >= S) return;
    const double z = lr_rank_z(R[jb * S + i], S);
    const int64_t t = i / C, c = i - t * C;
    const int64_t o = c * h2 + t;
    V[((FOLD ? 1 : 0) * pb + jb) * S + o] = z;
    if (!FOLD) {
        const uint64_t* q = Q + jb * kRankQ;
        const uint64_t u = U[jb * S + i];
        V[(2 * pb + jb) * S + o] = u <= q[4] ? 1.0 : 0.0;
        V[(3 * pb + jb) * S + o] = u <= q[5] ? 1.0 : 0.0;
    }
    if (z_out) z_out[i] = z;
}

// grid (M, 4 pb).  A [4 pb][L + 2][M]: row 0 the chain's mean, row 1 + l its acov(l) (zf, series 1: lag 0 alone, the rest 0).
__global__ void __launch_bounds__(256) k_rank_lag(const double* __restrict__ V, int64_t h, int64_t M, int pb, int L, double* __restrict__ A) {
    __shared__ double w[kRankLagSteps + kRankMaxLag + 1];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x, y = blockIdx.y;
    const int Lk = (int)(y / pb) == 1 ? 0 : L;
    const double* v = V + y * (h * M) + m * h;
    const double piv = v[0];
    double s = 0.0;
    for (int64_t t = tid; t < h; t += 256) s += v[t] - piv;
    red[tid] = s;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    const double dbar = red[0] / (double)h;
    double acc = 0.0;
    for (int64_t t0 = 0; t0 < h; t0 += kRankLagSteps) {
        const int64_t left = h - t0;
        const int nload = left < kRankLagSteps + Lk ? (int)left : kRankLagSteps + Lk;
        for (int q = tid; q < nload; q += 256) w[q] = (v[t0 + q] - piv) - dbar;
        __syncthreads();
        if (tid <= Lk) {
            const int64_t room = left - tid;  // products e_t e_{t+l} with t >= t0 that exist
            const int tend = room < kRankLagSteps ? (int)room : kRankLagSteps;
            for (int t = 0; t < tend; ++t) acc = __builtin_fma(w[t], w[t + tid], acc);
        }
        __syncthreads();
    }
    double* a = A + y * (int64_t)(L + 2) * M + m;
    if (tid <= L) a[(int64_t)(1 + tid) * M] = tid <= Lk ? acc / (double)h : 0.0;
    if (tid == 0) a[0] = piv + dbar;
}

// grid (ceil(M / 256), L + 3, 4 pb).  Row 0: sum of (mean_m - mean_0), row 1: of its square, row 2 + l: of acov_m(l).  part [4 pb][L + 3][nblk]
__global__ void __launch_bounds__(256) k_rank_partial(const double* __restrict__ A, int64_t M, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * 256 + tid, r = blockIdx.y, rows = gridDim.y, y = blockIdx.z;
    const double* a = A + y * (rows - 1) * M;
    double v = 0.0;
    if (m < M) {
        if (r < 2) {
            const double d = a[m] - a[0];
            v = r == 0 ? d : d * d;
        } else {
            v = a[(r - 1) * M + m];
        }
    }
    red[tid] = v;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    if (tid == 0) part[(y * rows + r) * gridDim.x + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) k_rank_final(const double* __restrict__ part, int64_t nblk, int64_t cells, double* __restrict__ tab) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    double s = part[e * nblk];
    for (int64_t b = 1; b < nblk; ++b) s += part[e * nblk + b];
    tab[e] = s;
}

}  // namespace lr
