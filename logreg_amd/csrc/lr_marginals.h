// lr_marginals.h -- the streaming marginal accumulator of include/logreg_hip_marginals.h: blocks [k][C][p] of draws in time order ->
// per coordinate a histogram of B + 3 columns (underflow, B bins, overflow, NaN) pooled over chains and time, and per series (chain,
// coordinate) the smallest and largest non-NaN draw and the power sums S1..S4 of u = (x - c_j) s_j.
//
// State:   counts [p][B+3] uint64 (pooled)        sums [NS][4], mn [NS], mx [NS] float64 per series s = c p + j (NS = C p)
//          grid [5][p] float64: lo, invw = B / (hi - lo), c = (lo + hi) / 2, s = 2 / (hi - lo), hi, all computed on the host
//
// k_marg_accumulate.  One lane per series, a workgroup of 256 lanes, the lane's coordinate fixed for the launch.  The lane walks the k
// time steps of the block, eight loads in flight, with its four sums, its min and its max in registers (one add / fma per draw and sum,
// in time order: the sums are the same bytes however the draws were cut into calls), and bumps a 32-bit counter of the workgroup's LDS
// table [rows][B+3] with an LDS integer atomic.  At the end of the launch the workgroup adds its non-zero counters to the global
// uint64 table with 64-bit integer atomics (exact in any order).  A launch folds at most kMargMaxSteps time steps: a counter holds at
// most 256 kMargMaxSteps = 2^28 < 2^32 and cannot wrap.
// Two lane maps, chosen on the host by the size of the table (marg_rows):
//     flat    p (B+3) 4 bytes fit the LDS budget: series s = 256 blockIdx + lane of the flattened axis (a time row is read fully
//             coalesced), LDS row = j = s % p.
//     tiled   otherwise the coordinates are cut into tiles of pt (a power of two, pt (B+3) 4 bytes within the budget): a workgroup takes
//             coordinates j0 .. j0 + pt - 1 of 256 / pt consecutive chains, lane = (chain, j - j0), LDS row = j - j0; a time row is
//             read in segments of pt values.
// k_marg_init sets the state of no draws (sums 0, mn +inf, mx -inf, counts 0).  k_marg_partial / k_marg_final merge the six per-series
// values over the chains: a fixed tree inside a workgroup of 256 chains, the workgroups in order; rows 0 and 1 by comparison (the state
// never holds a NaN: a NaN draw loses every comparison), rows 2..5 by addition.  No float atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lr {

constexpr int kMargMaxBins = 1024;
constexpr int kMargBlock = 256;
constexpr int kMargRows = 6;                  // min, max, S1..S4
constexpr int kMargLdsBytes = 48 * 1024;      // the budget of the counter table
constexpr int64_t kMargMaxSteps = 1 << 20;    // time steps per launch: 256 lanes x 2^20 steps < 2^32 per counter

// coordinates per LDS table: p itself when the whole table fits (flat), else the largest power of two that does (tiled, <= 256)
__host__ __device__ inline int marg_rows(int p, int bins) {
    const int fit = kMargLdsBytes / (4 * (bins + 3));
    if (p <= fit) return p;
    int pt = 1;
    while (2 * pt <= fit && 2 * pt <= kMargBlock) pt *= 2;
    return pt;
}

template <typename T>
__global__ void __launch_bounds__(kMargBlock) k_marg_accumulate(const T* __restrict__ block, int64_t k, int64_t C, int p, int bins, int pt,
                                                                const double* __restrict__ grid, unsigned long long* __restrict__ counts,
                                                                double* __restrict__ sums, double* __restrict__ mn, double* __restrict__ mx) {
#pragma clang fp contract(off)  // S1 += (x - c) s must stay a product and a sum
    extern __shared__ unsigned int tab[];  // [rows][bins + 3]
    const int tid = threadIdx.x;
    const int cols = bins + 3;
    const int64_t NS = C * p;
    int64_t s;
    int j, row, j0, rows;
    bool live;
    if (pt == p) {  // flat
        s = (int64_t)blockIdx.x * kMargBlock + tid;
        live = s < NS;
        j = (int)(s % p);
        row = j;
        j0 = 0;
        rows = p;
    } else {  // tiled: blockIdx = chain group x tile
        const int ntile = (p + pt - 1) / pt;
        const int tile = (int)(blockIdx.x % (unsigned)ntile);
        const int64_t c = (int64_t)(blockIdx.x / (unsigned)ntile) * (kMargBlock / pt) + tid / pt;
        j0 = tile * pt;
        row = tid % pt;
        j = j0 + row;
        live = c < C && j < p;
        s = c * p + j;
        rows = p - j0 < pt ? p - j0 : pt;
    }
    for (int i = tid; i < rows * cols; i += kMargBlock) tab[i] = 0u;
    __syncthreads();
    if (live) {
        const double lo = grid[j], invw = grid[p + j], ctr = grid[2 * p + j], scl = grid[3 * p + j], hi = grid[4 * p + j];
        const double nb = (double)bins;
        unsigned int* my = tab + row * cols;
        double S1 = sums[4 * s], S2 = sums[4 * s + 1], S3 = sums[4 * s + 2], S4 = sums[4 * s + 3];
        double lowest = mn[s], highest = mx[s];
        const T* src = block + s;
        auto fold = [&](double x) {
#pragma clang fp contract(off)
            const double t = (x - lo) * invw;
            const double tin = t >= 0.0 && t < nb ? t : 0.0;  // (only a value in range is converted)
            int col = 1 + (int)tin;                           // 0 <= t < bins: floor(t) = (int)t
            col = t >= nb || x >= hi ? bins + 1 : col;
            col = t < 0.0 ? 0 : col;
            col = x != x ? bins + 2 : col;
            atomicAdd(my + col, 1u);
            lowest = x < lowest ? x : lowest;
            highest = x > highest ? x : highest;
            const double u = (x - ctr) * scl;
            const double uu = u * u;
            S1 += u;
            S2 = __builtin_fma(u, u, S2);
            S3 = __builtin_fma(uu, u, S3);
            S4 = __builtin_fma(uu, uu, S4);
        };
        int64_t t = 0;
        for (; t + 8 <= k; t += 8) {
            T x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = src[(t + i) * NS];
#pragma unroll
            for (int i = 0; i < 8; ++i) fold((double)x[i]);
        }
        for (; t < k; ++t) fold((double)src[t * NS]);
        sums[4 * s] = S1;
        sums[4 * s + 1] = S2;
        sums[4 * s + 2] = S3;
        sums[4 * s + 3] = S4;
        mn[s] = lowest;
        mx[s] = highest;
    }
    __syncthreads();
    unsigned long long* out = counts + (int64_t)j0 * cols;
    for (int i = tid; i < rows * cols; i += kMargBlock) {
        const unsigned int v = tab[i];
        if (v) __hip_atomic_fetch_add(out + i, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the state of no draws; cells = p (bins + 3)
__global__ void __launch_bounds__(256) k_marg_init(int64_t NS, int64_t cells, unsigned long long* __restrict__ counts, double* __restrict__ sums,
                                                   double* __restrict__ mn, double* __restrict__ mx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cells) counts[i] = 0ull;
    if (i < NS) {
        sums[4 * i] = sums[4 * i + 1] = sums[4 * i + 2] = sums[4 * i + 3] = 0.0;
        mn[i] = __builtin_inf();
        mx[i] = -__builtin_inf();
    }
}

// a < b ? a : b for row 0, a > b ? a : b for row 1, a + b for the sums
__device__ inline double marg_merge(int r, double a, double b) { return r == 0 ? (b < a ? b : a) : r == 1 ? (b > a ? b : a) : a + b; }
__device__ inline double marg_identity(int r) { return r == 0 ? __builtin_inf() : r == 1 ? -__builtin_inf() : 0.0; }

// grid (ceil(C / 256), 6): a fixed tree over the 256 chains of a workgroup, per coordinate.  part [gridDim.x][6][p]
__global__ void __launch_bounds__(256) k_marg_partial(const double* __restrict__ sums, const double* __restrict__ mn, const double* __restrict__ mx,
                                                      int64_t C, int p, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 256 + tid;
    for (int j = 0; j < p; ++j) {
        const int64_t s = c * p + j;
        double v = marg_identity(r);
        if (c < C) v = r == 0 ? mn[s] : r == 1 ? mx[s] : sums[4 * s + (r - 2)];
        red[tid] = v;
        __syncthreads();
        for (int half = 128; half >= 1; half >>= 1) {
            if (tid < half) red[tid] = marg_merge(r, red[tid], red[tid + half]);
            __syncthreads();
        }
        if (tid == 0) part[((int64_t)blockIdx.x * kMargRows + r) * p + j] = red[0];
        __syncthreads();
    }
}

// one thread per (row, coordinate): the workgroups' partials merged in workgroup order
__global__ void __launch_bounds__(256) k_marg_final(const double* __restrict__ part, int64_t nblocks, int p, double* __restrict__ table) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cells = (int64_t)kMargRows * p;
    if (e >= cells) return;
    const int r = (int)(e / p);
    double v = part[e];
    for (int64_t b = 1; b < nblocks; ++b) v = marg_merge(r, v, part[b * cells + e]);
    table[e] = v;
}

}  // namespace lr
