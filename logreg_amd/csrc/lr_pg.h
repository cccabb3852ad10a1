// lr_pg.h -- the fused many-chain Polya-Gamma Gibbs sampler: one launch runs `iters x thin` sweeps for every chain
// (include/logreg_hip_pg.h: the sweep, the draw, its random stream and the bound of every loop).
//
// Layout as k_nuts (lr_nuts.h): one chain per 16-lane DPP row, rows staged in LDS, lane r owns coordinates r + 16 k.  A sweep has two
// phases.  Phase 1: the 16 lanes deal the rows round-robin; a lane forms psi_i from the gathered state, draws omega_i from the row's
// own Philox sub-stream and stages it in LDS behind the rows ([16 chains][n] of T).  Phase 2: lane r owns ROWS r + 16 k of the
// symmetric matrix A (all P columns, in registers, every index a compile-time constant) and sums over the data rows in row order;
// the unit-diagonal scaling, the Cholesky factorisation (right-looking, column k's multipliers broadcast with row_share DPP moves),
// the forward solve (column-oriented) and the backward solve (one group_sum<16> per coordinate) run distributed over the same 16
// lanes in float64.  No LDS workspace, no runtime-indexed register array.
//
// Every loop of the draw has a compile-time trip bound and every comparison reads a NaN as false: no value can hang a lane.
#pragma once

#include <type_traits>

#include "lr_nuts.h"  // nuts_gather_small

namespace lr {

constexpr uint32_t TAG_PG = 0x10000000u;  // | b << 16 | row: block b of the row's sub-stream (LR_PG_TAG)
constexpr int kPgMaxRounds = 10, kPgMaxTrials = 160, kPgMaxTerms = 8;
constexpr int kKindPg = 6;  // LR_KIND_PG

// f(integral_constant<int, I>) for I = LO .. HI - 1: loops whose index must be a constant expression (DPP controls, register arrays)
template <int LO, int HI, class F> __device__ __forceinline__ void pg_static_for(F&& f) {
    if constexpr (LO < HI) {
        f(std::integral_constant<int, LO>{});
        pg_static_for<LO + 1, HI>(f);
    }
}

struct PgCounters {  // lr_pg_counters
    uint64_t proposals, series_terms;
    uint32_t skipped, reserved;
};

template <typename T, int P> struct PgArgs {
    T* state;              // [C][p] in/out (read only with omega_out)
    T* out;                // [iters][C][p] or null
    PgCounters* counters;  // [C] added to, or null
    T* omega_out;          // [C][n]: lr_pg_omega -- phase 1 of ONE sweep, nothing else is written; else null
    int64_t C, chain_offset, iters, thin, iter_offset;
    uint64_t seed;
    int p;
    double b[P];     // X^T (y - 1/2), zero in padded coordinates
    double ivar[P];  // 1 / pscale^2, ONE in padded coordinates (the padded block of A is the identity)
    StatsArgs stats;
};

// dynamic LDS of k_pg beyond the rows: the omega of the 16 chains of a workgroup
template <typename T> constexpr size_t pg_stage_bytes(int64_t n) { return (size_t)16 * (size_t)n * sizeof(T); }

__device__ __forceinline__ float pg_log(float x) { return logf(x); }
__device__ __forceinline__ double pg_log(double x) { return log(x); }
__device__ __forceinline__ float pg_exp(float x) { return expf(x); }
__device__ __forceinline__ double pg_exp(double x) { return exp(x); }
__device__ __forceinline__ float pg_erfc(float x) { return erfcf(x); }
__device__ __forceinline__ double pg_erfc(double x) { return erfc(x); }
__device__ __forceinline__ float pg_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double pg_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float pg_cospi(float x) { return cospif(x); }
__device__ __forceinline__ double pg_cospi(double x) { return cospi(x); }

// the words of a row's sub-stream, in order
struct PgWords {
    uint32_t c0, c1, c2, k0, k1, row;
    uint32_t cursor;
    U4 blk;
    __device__ __forceinline__ uint32_t next() {
        const uint32_t w = cursor & 3u;
        if (w == 0) blk = philox4x32_10(c0, c1, c2, TAG_PG | ((cursor >> 2) << 16) | row, k0, k1);
        ++cursor;
        return w == 0 ? blk.x : (w == 1 ? blk.y : (w == 2 ? blk.z : blk.w));
    }
};

// a_n(x) (include/logreg_hip_pg.h)
template <typename T> __device__ __forceinline__ T pg_coef(int n, T x, bool small) {
    constexpr T kPi = T(3.14159265358979323846);
    const T h = T(n) + T(0.5);
    if (small) {
        const T v = T(2) / (kPi * x);
        return kPi * h * (v * pg_sqrt(v)) * pg_exp(T(-2) * h * h / x);
    }
    return kPi * h * pg_exp(-(h * h) * (kPi * kPi * T(0.5)) * x);
}

// omega ~ PG(1, |psi|), psi finite; nprop / nterm gain the rounds and the series terms of the draw
template <typename T>
__device__ __forceinline__ T pg_draw(T psi, uint64_t seed, uint64_t gchain, uint64_t iter, uint32_t row, uint32_t& nprop, uint32_t& nterm) {
    constexpr T kPi = T(3.14159265358979323846), t = T(0.64), kInvT = T(1) / T(0.64), kSqrtT = T(0.8);
    const T z = T(0.5) * (psi < T(0) ? -psi : psi);
    const T K = kPi * kPi * T(0.125) + T(0.5) * z * z;
    T r = T(0);
    if (z < T(10)) {
        const T kt = K * t;
        const T pb = T(0.5) * pg_erfc(-((t * z - T(1)) / kSqrtT) * T(0.70710678118654752440));
        const T pa = T(0.5) * pg_erfc(((t * z + T(1)) / kSqrtT) * T(0.70710678118654752440));
        r = T(1) / (T(1) + (T(4) / kPi) * K * (pg_exp(kt - z) * pb + pg_exp(kt + z) * pa));
    }
    const bool pair = z < kInvT;
    const T mu = T(1) / z;  // (inf at z = 0: the pair method runs there)
    PgWords ws{(uint32_t)gchain, (uint32_t)iter, (uint32_t)(iter >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), row, 0u, U4{0, 0, 0, 0}};
    T X = t;
    for (int round = 0; round < kPgMaxRounds; ++round) {
        ++nprop;
        const T U = u01<T>(ws.next());
        if (U < r) {
            const T E = -pg_log(u01<T>(ws.next()));
            X = t + E / K;
        } else {
            for (int trial = 0; trial < kPgMaxTrials; ++trial) {
                const T ua = u01<T>(ws.next()), ub = u01<T>(ws.next()), uc = u01<T>(ws.next());
                bool ok;
                if (pair) {
                    const T E1 = -pg_log(ua), E2 = -pg_log(ub);
                    const T d = T(1) + t * E1;
                    X = t / (d * d);
                    ok = (E1 * E1 <= T(2) * E2 / t) && (uc <= pg_exp(T(-0.5) * z * z * X));
                } else {
                    const T N = pg_sqrt(T(-2) * pg_log(ua)) * pg_cospi(T(2) * ub);
                    const T w = T(0.5) * mu * (N * N);
                    const T s = T(1) + w + pg_sqrt(w * (w + T(2)));
                    X = mu / s;
                    if (uc > mu / (mu + X)) X = mu * s;
                    ok = X <= t;
                }
                if (ok) break;
                if (trial == kPgMaxTrials - 1) X = X > t ? t : X;
            }
        }
        const bool small = X <= t;
        const T V = u01<T>(ws.next());
        T S = pg_coef<T>(0, X, small);
        const T Y = V * S;
        bool accept = true;  // (at the series bound: accept)
        for (int n = 1; n <= kPgMaxTerms; ++n) {
            ++nterm;
            const T an = pg_coef<T>(n, X, small);
            if (n & 1) {
                S -= an;
                if (Y <= S) break;
            } else {
                S += an;
                if (Y > S) {
                    accept = false;
                    break;
                }
            }
        }
        if (accept) break;
    }
    return T(0.25) * X;
}

template <typename T> __device__ __forceinline__ bool pg_finite(T v) { return (v < T(0) ? -v : v) < T(__builtin_inf()); }

// The hyper-step hooks of pg_sweeps: none for k_pg.  lr_hs.h's HsState (kHyper = true) adds the horseshoe's prior precision to the diagonal
// of A, updates its scales after the back-solve and writes them out with a kept draw; every call site is under `if constexpr`, so k_pg's
// code does not depend on it.
struct PgNoHyper {
    static constexpr bool kHyper = false;
};

// `iters x thin` sweeps of every chain: the body of k_pg and of k_hs (lr_hs.h)
template <typename T, int P, class H>
__device__ __forceinline__ void pg_sweeps(const ModelArgs<T, P>& m, const PgArgs<T, P>& a, H& h) {
    constexpr int G = 16, NK = (P + 15) / 16, LD = P + kLdsRowPad<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int gl = threadIdx.x % G, r = threadIdx.x & 15;
    int64_t chain = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool live = chain < a.C;
    if (!live) chain = a.C - 1;  // whole waves stay converged for the DPP exchanges; stores are masked
    T* const rows = reinterpret_cast<T*>(smem_raw);
    (void)make_rows<T, P, G, MODE_LDS, 0>(m, gl, rows);  // stages the rows, pitch LD
    const int n = (int)m.n;
    T* const om = rows + (size_t)n * LD + (size_t)(threadIdx.x / G) * n;  // this chain's omega [n]
    const uint64_t gchain = (uint64_t)(a.chain_offset + chain);
    const int rz = r < P ? r : 0;

    T x[NK];
    double bown[NK], ivown[NK];
    int jown[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int j = r + 16 * k, js = j < P ? j : 0;
        jown[k] = js;
        x[k] = j < a.p ? a.state[chain * a.p + j] : T(0);
        bown[k] = j < P ? a.b[js] : 0.0;
        ivown[k] = j < P ? a.ivar[js] : 1.0;
    }
    uint64_t n_prop = 0, n_term = 0;
    uint32_t n_skip = 0;

    DrawBatch<T, P, G> draws;
    static_assert(DrawBatch<T, P, G>::kEnabled, "batched draws");
    draws.reset();
    const int64_t sweeps = a.omega_out ? 1 : a.iters * a.thin;
    for (int64_t sw = 0; sw < sweeps; ++sw) {
        const uint64_t iter = (uint64_t)(a.iter_offset + sw);
        // ---- phase 1: psi, the screen, the draws
        T xb[P];
        if constexpr (P >= 16) {
#pragma unroll
            for (int k = 0; k < NK; ++k) dist_gather16<T, P>(x[k], k, xb);
        } else {
            nuts_gather_small<T, P>(x[0], xb);
        }
        uint32_t prop_it = 0, term_it = 0;
        bool bad = false;
        for (int i = r; i < n; i += G) {
            const T* row = rows + (size_t)i * LD;
            T psi = T(0);
#pragma unroll
            for (int j = 0; j < P; ++j) psi = fma_t(row[j], xb[j], psi);
            const bool fin = pg_finite(psi);
            bad = bad || !fin;
            const T w = pg_draw<T>(fin ? psi : T(0), a.seed, gchain, iter, (uint32_t)i, prop_it, term_it);
            om[i] = w;
            if (a.omega_out && live) a.omega_out[chain * (int64_t)n + i] = fin ? w : T(__builtin_nan(""));
        }
        if (a.omega_out) return;
        bad = group_sum<16>(bad ? 1.0f : 0.0f) != 0.0f;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // ---- phase 2: A (rows r + 16 k), in row order
        double A[NK][P];
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int c = 0; c < P; ++c) A[k][c] = 0.0;
        for (int i = 0; i < n; ++i) {
            const T* row = rows + (size_t)i * LD;
            const double w = (double)om[i];
            double xr[P];
#pragma unroll
            for (int c = 0; c < P; ++c) xr[c] = (double)row[c];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const double xj = (double)row[jown[k]];
#pragma unroll
                for (int c = 0; c < P; ++c) A[k][c] = __builtin_fma(w, xj * xr[c], A[k][c]);
            }
        }
        __builtin_amdgcn_wave_barrier();  // (the next sweep's phase 1 overwrites om)
        // + prior on the diagonal; the diagonal itself
        double dj[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            double diag = 0.0;
            double prec = ivown[k];
            if constexpr (H::kHyper) prec = h.precision(k, ivown[k]);
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const bool mine = c == r + 16 * k;
                A[k][c] += mine ? prec : 0.0;
                diag += mine ? A[k][c] : 0.0;
            }
            dj[k] = 1.0 / sqrt(diag);  // (lanes beyond the padded width: 1 / sqrt(0), never read by a lane that matters)
        }
        // R = A (d d^T)
        pg_static_for<0, P>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            const double dc = dpp_mov<0x150 + (c & 15)>(dj[c >> 4]);
#pragma unroll
            for (int k = 0; k < NK; ++k) A[k][c] = A[k][c] * (dj[k] * dc);
        });
        // Cholesky, right-looking; rhs = D b solved on the way (L y = D b, column-oriented)
        double y[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) y[k] = dj[k] * bown[k];
        bool ok = true;
        pg_static_for<0, P>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            const double piv = dpp_mov<0x150 + (c & 15)>(A[c >> 4][c]);
            ok = ok && (piv > 0.0) && (piv < __builtin_inf());
            const double lcc = sqrt(piv);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const bool own = c == r + 16 * k;
                A[k][c] = own ? lcc : A[k][c] / lcc;  // L_jc
            }
            // y_c = rhs_c / L_cc at its owner; rows below: rhs_j -= L_jc y_c
            const double yc = dpp_mov<0x150 + (c & 15)>(y[c >> 4]) / lcc;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int j = r + 16 * k;
                y[k] = j == c ? yc : (j > c ? __builtin_fma(-A[k][c], yc, y[k]) : y[k]);
            }
            pg_static_for<c + 1, P>([&](auto c2c) {
                constexpr int c2 = decltype(c2c)::value;
                const double l2 = dpp_mov<0x150 + (c2 & 15)>(A[c2 >> 4][c]);  // L_{c2 c}
#pragma unroll
                for (int k = 0; k < NK; ++k) A[k][c2] = __builtin_fma(-A[k][c], l2, A[k][c2]);
            });
        });
        // L^T x = y + z, coordinate P - 1 first: x_c = (w_c - sum_{j > c} L_jc x_j) / L_cc
        T zt[NK], lu_unused;
        draws.template next_own<NK>(a.seed, gchain, iter, gl, rz, zt, lu_unused);
        double xs[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) xs[k] = y[k] + (double)zt[k];
        pg_static_for<0, P>([&](auto ci) {
            constexpr int c = P - 1 - decltype(ci)::value;
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < NK; ++k) part = (r + 16 * k > c && r + 16 * k < P) ? __builtin_fma(A[k][c], xs[k], part) : part;
            const double tot = group_sum<16>(part);
            const double lcc = dpp_mov<0x150 + (c & 15)>(A[c >> 4][c]);
#pragma unroll
            for (int k = 0; k < NK; ++k) xs[k] = (r + 16 * k == c) ? (xs[k] - tot) / lcc : xs[k];
        });
        const bool skip = bad || !ok;
#pragma unroll
        for (int k = 0; k < NK; ++k) x[k] = (skip || r + 16 * k >= a.p) ? x[k] : (T)(dj[k] * xs[k]);
        n_prop += skip ? 0u : prop_it;
        n_term += skip ? 0u : term_it;
        n_skip += skip ? 1u : 0u;
        if constexpr (H::kHyper) h.step(skip, x, iter);  // (A is dead here)

        if ((sw + 1) % a.thin == 0 && live) {
            const int64_t it = sw / a.thin;
            if constexpr (H::kHyper) h.keep(it);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int j = r + 16 * k;
                if (j < a.p) {
                    if (a.out) a.out[(it * a.C + chain) * a.p + j] = x[k];
                    if (a.stats.buf) {  // (stats_update of lr_device.h for one coordinate)
                        const int64_t idx = a.stats.first + it, bb = idx / a.stats.batch, kk = idx - bb * a.stats.batch;
                        double* sbuf = a.stats.buf + ((bb * a.C + chain) * 2) * a.p;
                        stats_fold(sbuf + j, sbuf + a.p + j, kk, 1.0 / (double)(kk + 1), (double)x[k]);
                    }
                }
            }
        }
    }
    // the chain's counters: the lanes' tallies summed (exact in a double)
    const double tp = group_sum<16>((double)n_prop), tt = group_sum<16>((double)n_term);
    if (live) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (r + 16 * k < a.p) a.state[chain * a.p + r + 16 * k] = x[k];
        if (r == 0 && a.counters) {
            PgCounters* cn = a.counters + chain;
            cn->proposals += (uint64_t)tp;
            cn->series_terms += (uint64_t)tt;
            cn->skipped += n_skip;
        }
    }
}

template <typename T, int P>
__global__ void __launch_bounds__(256) k_pg(ModelArgs<T, P> m, PgArgs<T, P> a) {
    PgNoHyper h;
    pg_sweeps<T, P>(m, a, h);
}

}  // namespace lr
