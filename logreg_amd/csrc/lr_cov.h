// lr_cov.h -- the streaming second cross-moment of include/logreg_hip_cov.h: blocks [k][C][p] of draws in time order -> per chain the
// sums S[c][j] of u_j = (x_j - center_j) scale_j and, per cell of the header's partition (chain group g = c / G, time residue r = t mod R),
// the upper triangle of sum u u^T.
//
// State:   cells [ncell][E] float64, cell = g R + r, E = NT T T: the NT = nb (nb + 1) / 2 tiles (bi <= bj, row-major) of T x T entries,
//          entry (bi T + a, bj T + b) at tile T T + a T + b (a diagonal tile holds both halves; the host reads a <= b)
//          chain sums [C][p] float64          cs [2][p] float64: center, scale
//
// k_cov_accumulate<T, P>.  A workgroup of 256 lanes per chain group.  A lane owns one tile of one time residue: lane = r NT + tile (R NT
// <= 256), its T x T accumulators in registers from the first draw of the launch to the last (nothing indexed at run time).  The launch
// walks its k time steps in windows of R; per window the group's chains go by in chunks of GC: the chunk's draws of the window are
// converted once to u in float64 and staged in LDS [R][GC][P]; the first GC p lanes add the chunk's u to the chain sums in time order;
// then every lane whose residue has a time step in the window takes the chunk's chains in order, 2 T LDS reads and T T fma per draw.
// Window outside, chunk inside, chain innermost: a cell sees its draws in (t, c) order whatever k is, and the absolute time of the
// launch's first step (the accumulator's count) decides which residue a step belongs to.
// k_cov_runs adds runs of consecutive rows of a table [rows][E] one after the other, k_cov_outer forms the chain_outer / sum partials
// of runs of chains; lr_cov_result applies k_cov_runs twice (runs of rows, then all runs).  No float atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lr {

constexpr int kCovBlock = 256;
constexpr int kCovCellRun = 64;    // LR_COV_CELL_RUN
constexpr int kCovOuterRun = 128;  // LR_COV_OUTER_RUN

__host__ __device__ constexpr int cov_tile(int P) { return P / 4 < 8 ? P / 4 : 8; }
__host__ __device__ constexpr int cov_nb(int P) { return P / cov_tile(P); }
__host__ __device__ constexpr int cov_ntiles(int P) { return cov_nb(P) * (cov_nb(P) + 1) / 2; }
__host__ __device__ constexpr int cov_residues(int P) { return kCovBlock / cov_ntiles(P); }              // 25, 25, 25, 25, 7, 1
__host__ __device__ constexpr int cov_chunk(int P) { return P <= 32 ? 128 / P : P == 64 ? 8 : 32; }       // chains staged together
__host__ __device__ constexpr int cov_groups(int P) { return P == 4 ? 4096 : P == 8 ? 2048 : P == 16 ? 1024 : 512; }
__host__ __device__ constexpr int cov_entries(int P) { return cov_ntiles(P) * cov_tile(P) * cov_tile(P); }  // doubles per cell

// chains per group: the chunk doubled until ceil(C / G) groups are within cov_groups(P)
__host__ __device__ inline int64_t cov_group_chains(int64_t C, int P) {
    int64_t G = cov_chunk(P);
    while ((C + G - 1) / G > cov_groups(P)) G *= 2;
    return G;
}

template <typename T, int P>
__global__ void __launch_bounds__(kCovBlock) k_cov_accumulate(const T* __restrict__ block, int64_t k, int64_t t0, int64_t C, int p, int64_t G,
                                                              const double* __restrict__ cs, double* __restrict__ cells,
                                                              double* __restrict__ chain_sums) {
#pragma clang fp contract(off)  // u = (x - c) s and S += u stay a difference, a product and a sum; the moment's fma is spelled out
    constexpr int TL = cov_tile(P), NB = cov_nb(P), NT = cov_ntiles(P), R = cov_residues(P), GC = cov_chunk(P), E = cov_entries(P);
    static_assert(R * NT <= kCovBlock && P % TL == 0 && R * GC * P * 8 <= 32 * 1024, "lane map and LDS budget");
    __shared__ double u[R * GC * P];  // [slot of the window][chain of the chunk][coordinate]
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t c_first = g * G;
    const int64_t c_end = c_first + G < C ? c_first + G : C;
    const bool owner = tid < R * NT;
    const int r = owner ? tid / NT : 0;
    int bi = 0, bj = tid % NT;  // tile -> (bi, bj), bi <= bj, row-major over the upper triangle
    while (bj >= NB - bi) {
        bj -= NB - bi;
        ++bi;
    }
    bj += bi;
    const int slot = (int)(((r - t0) % R + R) % R);  // the window slot whose absolute time is r mod R
    double* mine = cells + ((size_t)g * R + r) * E + (size_t)(tid % NT) * TL * TL;
    double acc[TL][TL];
    if (owner) {
#pragma unroll
        for (int a = 0; a < TL; ++a)
#pragma unroll
            for (int b = 0; b < TL; ++b) acc[a][b] = mine[a * TL + b];
    }
    // the lane's coordinate when it stages (GC P divides or is a multiple of 256: j is fixed when P <= 256) and its centre and scale
    const int js = tid % P;
    const double ctr = js < p ? cs[js] : 0.0, scl = js < p ? cs[p + js] : 0.0;
    for (int64_t w0 = 0; w0 < k; w0 += R) {
        const int wlen = k - w0 < R ? (int)(k - w0) : R;
        for (int64_t c0 = c_first; c0 < c_end; c0 += GC) {
            const int nc = c_end - c0 < GC ? (int)(c_end - c0) : GC;
            for (int e = tid; e < R * GC * P; e += kCovBlock) {  // (256 is a multiple of P or P of 256... P <= 128: e % P == js)
                const int ti = e / (GC * P), c = (e / P) % GC;
                double v = 0.0;
                if (ti < wlen && c < nc && js < p) v = ((double)block[((w0 + ti) * C + c0 + c) * p + js] - ctr) * scl;
                u[e] = v;
            }
            __syncthreads();
            for (int e = tid; e < GC * P; e += kCovBlock) {  // the chain sums of the chunk, in time order
                const int c = e / P;
                if (c < nc && js < p) {
                    double s = chain_sums[(c0 + c) * p + js];
                    for (int ti = 0; ti < wlen; ++ti) s += u[ti * GC * P + e];
                    chain_sums[(c0 + c) * p + js] = s;
                }
            }
            if (owner && slot < wlen) {
                const double* row = u + slot * GC * P;
                for (int c = 0; c < nc; ++c) {
                    double x[TL], y[TL];
#pragma unroll
                    for (int a = 0; a < TL; ++a) x[a] = row[c * P + bi * TL + a];
#pragma unroll
                    for (int b = 0; b < TL; ++b) y[b] = row[c * P + bj * TL + b];
#pragma unroll
                    for (int a = 0; a < TL; ++a)
#pragma unroll
                        for (int b = 0; b < TL; ++b) acc[a][b] = __builtin_fma(x[a], y[b], acc[a][b]);
                }
            }
            __syncthreads();
        }
    }
    if (owner) {
#pragma unroll
        for (int a = 0; a < TL; ++a)
#pragma unroll
            for (int b = 0; b < TL; ++b) mine[a * TL + b] = acc[a][b];
    }
}

// the state of no draws
__global__ void __launch_bounds__(256) k_cov_init(double* __restrict__ state, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) state[i] = 0.0;
}

// grid (ceil(E / 256), ceil(rows / run)): out [run index][E] = the rows of one run of in [rows][E], added one after the other
__global__ void __launch_bounds__(256) k_cov_runs(const double* __restrict__ in, int64_t rows, int64_t E, int64_t run, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t first = (int64_t)blockIdx.y * run;
    const int64_t last = first + run < rows ? first + run : rows;
    double v = in[first * E + e];
    for (int64_t q = first + 1; q < last; ++q) v += in[q * E + e];
    out[(int64_t)blockIdx.y * E + e] = v;
}

// grid (ceil(C / kCovOuterRun), ceil((p p + p) / 256)): out [run][p p + p]: entries i p + j, i <= j, the run's sum of S_ci S_cj (one fma per
// chain in chain order; i > j is left 0), then p entries: the run's sum of S_cj
__global__ void __launch_bounds__(256) k_cov_outer(const double* __restrict__ S, int64_t C, int p, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int pp = p * p;
    if (e >= pp + p) return;
    const int64_t first = (int64_t)blockIdx.x * kCovOuterRun;
    const int64_t last = first + kCovOuterRun < C ? first + kCovOuterRun : C;
    double v = 0.0;
    if (e < pp) {
        const int i = e / p, j = e % p;
        if (i <= j)
            for (int64_t c = first; c < last; ++c) v = __builtin_fma(S[c * p + i], S[c * p + j], v);
    } else {
        const int j = e - pp;
        v = S[first * p + j];
        for (int64_t c = first + 1; c < last; ++c) v += S[c * p + j];
    }
    out[(int64_t)blockIdx.x * (pp + p) + e] = v;
}

}  // namespace lr
