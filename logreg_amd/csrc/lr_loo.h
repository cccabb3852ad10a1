// lr_loo.h -- PSIS-LOO of include/logreg_hip_loo.h: draws beta_s [S][P] -> the matrix of pointwise log-likelihoods l[i][s] of the model's
// own rows (k_loo_fill), and per observation the Pareto-smoothed leave-one-out estimate with its k-hat (k_psis).
//
// Layout of the matrix: [n][ld], an observation's draws contiguous (ld = max_draws rounded up to 128 bytes) -- the PSIS stage walks a
// row of it five to ten times with consecutive lanes on consecutive addresses.  The fill writes by (draw, row): a lane owns a row (its
// x_i in registers, the draws arriving through the scalar unit: pred_eta / pred_pair of lr_predict.h, unchanged) and would store with a
// stride of ld, so a workgroup collects kLooTile = 128 bytes' worth of draws for its 256 rows in LDS and writes them out transposed, one
// full 128-byte line per row and pass.  A caller's matrix [S][r] (lr_psis) and the matrix handed back (lr_loo_loglik) go through
// k_loo_transpose, tiles of 32 x 32 through LDS.
//
// k_psis.  A workgroup per observation, NT lanes, the row l_s (s < S) read as it is stored and widened exactly to float64.
//   1  one pass: the smallest l (a = -min l), whether anything is not finite (then the five outputs are NaN), and the OR / AND of the
//      order-preserving integer keys: the bits on which the keys agree need no selection pass
//   2  exact radix select of the (M + 1)-th smallest l on the keys, 11 bits a pass from the highest bit that differs: LDS histogram by
//      integer atomics, a scan over the bins, the digit that holds the rank.  v = -l - a falls as l grows and rounding keeps the order,
//      so c = -l* - a IS the (S - M)-th smallest v; the tail {v_s > c} is decided on the float64 v (ties by rounding included)
//   3  one pass: the tail's v into LDS (slots by an integer atomic; the order is arbitrary), and over everything else the sums of
//      exp(v) and exp(v)^2; over every draw the sum of exp(l).  Then a bitonic sort of the tail in LDS: from here on nothing depends on
//      the order the slots were taken in
//   4  the generalised-Pareto fit on x_j = exp(v_(j)) - exp(c): theta_j by lane j; k_j by a wave per j (lanes stride the tail, a
//      butterfly over the wave); omega_j by lane j; theta, k, sigma by workgroup sums
//   5  the smoothed (or raw) tail weights and the closed-form sums
// Every float64 sum: a lane adds its elements in index order, a xor-butterfly over the wave (both partners compute the same sum), the
// waves' sums in wave order -- a fixed tree for a given (NT, S); products inside sums are spelled fma, contraction is off.  No float
// atomics, no private arrays, nothing goes back to the host per row.
// LDS: the sort buffer (CAP doubles, CAP a power of two), x (CAP doubles, the select's histogram lives there before x does), a few
// hundred bytes of reduction slots.  Two sizes: CAP = 1024 for S <= kLooSmallDraws (M <= 768; 19 KB, NT = 256) and CAP = 4096 (M <= 3072:
// S <= kLooMaxDraws = 2^20; x keeps 3072 slots; 59 KB, NT = 512: 1024 lanes would leave 128 registers a lane, too few).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_predict.h"

namespace lr {

constexpr int kLooRows = 5;
constexpr int kLooBlock = 256;                 // lanes = rows per workgroup of k_loo_fill
constexpr int kLooTileBytes = 128;             // draws collected per row before a write-out
constexpr int kLooDigit = 11;                  // bits per selection pass
constexpr int kLooBins = 1 << kLooDigit;
constexpr int kLooFitMax = 96;                 // m = 30 + floor(sqrt(n_t)) <= 30 + 55
constexpr int64_t kLooMaxDraws = 1 << 20;      // M(2^20) = 3072
constexpr int64_t kLooSmallDraws = 1 << 16;    // M(2^16) = 768

// M = min(floor(S / 5), m3), m3 = the smallest integer with m3^2 >= 9 S -- in integers
__host__ inline int64_t loo_tail_len(int64_t S) {
    if (S <= 0) return 0;
    int64_t m3 = 0;
    while (m3 * m3 < 9 * S) m3 += 1024;
    while (m3 > 0 && (m3 - 1) * (m3 - 1) >= 9 * S) --m3;
    return S / 5 < m3 ? S / 5 : m3;
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------------
// rows [n][P] signed rows; draws [S][P]; slice y takes draws [y per, min(S, (y + 1) per)), per a multiple of the tile; ll [n][ld], the
// draws land at columns n0 + s.  Lanes past the last row redo it and store nothing.
template <typename T, int P>
__global__ void __launch_bounds__(kLooBlock) k_loo_fill(const T* __restrict__ rows, int64_t n, const T* __restrict__ draws, int64_t S, int64_t per,
                                                        T* __restrict__ ll, int64_t ld, int64_t n0) {
    constexpr int CH = PredGeom<T, P>::CH, NCH = PredGeom<T, P>::NCH, DG = PredGeom<T, P>::DG;
    constexpr int TS = kLooTileBytes / (int)sizeof(T), LDT = TS + 1, RPP = kLooBlock / TS;  // rows per write-out pass
    __shared__ T tile[kLooBlock * LDT];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kLooBlock + tid;
    const int64_t il = i < n ? i : n - 1;
    const T* __restrict__ xrow = rows + il * P;
    T x[CH];
    if constexpr (NCH == 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) x[j] = xrow[j];
    }
    const int64_t s0 = (int64_t)blockIdx.y * per, s1 = s0 + per < S ? s0 + per : S;
    T* __restrict__ mine = tile + tid * LDT;
    for (int64_t s = s0; s < s1; s += TS) {
        const int cnt = s1 - s < TS ? (int)(s1 - s) : TS;
        int d = 0;
        for (; d + DG <= cnt; d += DG) {
            T eta[DG];
            pred_eta<T, P, DG>(xrow, x, draws + (s + d) * P, eta);
#pragma unroll
            for (int g = 0; g < DG; ++g) {
                T pi, L, l;
                pred_pair<T>(eta[g], true, pi, L, l);
                mine[d + g] = l;
            }
        }
        for (; d < cnt; ++d) {
            T eta[1];
            pred_eta<T, P, 1>(xrow, x, draws + (s + d) * P, eta);
            T pi, L, l;
            pred_pair<T>(eta[0], true, pi, L, l);
            mine[d] = l;
        }
        __syncthreads();
        const int dd = tid % TS;
#pragma unroll 4
        for (int pass = 0; pass < TS; ++pass) {
            const int rl = pass * RPP + tid / TS;
            const int64_t gi = (int64_t)blockIdx.x * kLooBlock + rl;
            if (gi < n && dd < cnt) ll[gi * ld + n0 + s + dd] = tile[rl * LDT + dd];
        }
        __syncthreads();
    }
}

// src [A][lds] -> dst [B][ldd], dst[b][a] = src[a][b] for a < A, b < B.  grid (ceil(A / 32), ceil(B / 32)), block (32, 8)
template <typename T>
__global__ void __launch_bounds__(256) k_loo_transpose(const T* __restrict__ src, int64_t A, int64_t B, int64_t lds, T* __restrict__ dst, int64_t ldd) {
    __shared__ T t[32][33];
    const int64_t a0 = (int64_t)blockIdx.x * 32, b0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int64_t a = a0 + ty + k, b = b0 + tx;
        if (a < A && b < B) t[ty + k][tx] = src[a * lds + b];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int64_t b = b0 + ty + k, a = a0 + tx;
        if (a < A && b < B) dst[b * ldd + a] = t[tx][ty + k];
    }
}

// ---- PSIS -----------------------------------------------------------------------------------------------------------------------------
// order-preserving keys: key(x) < key(y) <=> x < y for non-NaN x, y (-0 sorts below +0; both give the same v)
template <typename T> struct LooKey;
template <> struct LooKey<float> {
    using U = uint32_t;
    static constexpr int BITS = 32;
    __device__ static __forceinline__ U of(float x) {
        const U u = __float_as_uint(x);
        return (u >> 31) ? ~u : (u | 0x80000000u);
    }
    __device__ static __forceinline__ float from(U k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }
};
template <> struct LooKey<double> {
    using U = unsigned long long;
    static constexpr int BITS = 64;
    __device__ static __forceinline__ U of(double x) {
        const U u = (U)__double_as_longlong(x);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    __device__ static __forceinline__ double from(U k) { return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k)); }
};

// a value per lane -> the same combination in every lane of the workgroup: butterfly over the wave, the waves in wave order.
// buf: NT / 64 slots of LDS, free on entry (two barriers inside)
template <int NT, typename V, typename F>
__device__ __forceinline__ V loo_block_red(V v, F f, V* buf) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = f(v, (V)__shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    V t = buf[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t = f(t, buf[w]);
    __syncthreads();
    return t;
}
template <int NT>
__device__ __forceinline__ double loo_block_sum(double v, double* buf) {
    return loo_block_red<NT>(v, [](double a, double b) { return a + b; }, buf);
}

// ll [r][ld]: row blockIdx.x holds S draws.  M = loo_tail_len(S) (<= XCAP).  table [kLooRows][r].
template <typename T, int NT, int CAP, int XCAP>
__global__ void __launch_bounds__(NT) k_psis(const T* __restrict__ ll, int64_t ld, int S, int M, int64_t r, double* __restrict__ table) {
#pragma clang fp contract(off)
    using K = LooKey<T>;
    using U = typename K::U;
    constexpr int NW = NT / 64, BPT = kLooBins / NT;
    static_assert(kLooBins % NT == 0 && XCAP * 8 >= kLooBins * 4 && XCAP <= CAP, "LDS plan");
    __shared__ double tail[CAP];
    __shared__ double xs[XCAP];
    __shared__ double dred[NW];
    __shared__ U ured[NW];
    __shared__ unsigned wtot[NW];
    __shared__ unsigned sel[2];
    __shared__ unsigned ntail;
    __shared__ double th[kLooFitMax], kk[kLooFitMax], LL[kLooFitMax];
    unsigned* const hist = reinterpret_cast<unsigned*>(xs);  // dead before xs is written
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* __restrict__ row = ll + (int64_t)blockIdx.x * ld;
    double* __restrict__ out = table + blockIdx.x;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    // 1: the smallest l, non-finite values, the bits on which the keys differ
    U kmin = ~U(0), kor = U(0), kand = ~U(0);
    int bad = 0;
    for (int s = tid; s < S; s += NT) {
        const T x = row[s];
        bad |= !(__builtin_fabs((double)x) < inf);
        const U k = K::of(x);
        kmin = k < kmin ? k : kmin;
        kor |= k;
        kand &= k;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            for (int q = 0; q < kLooRows; ++q) out[q * r] = nan;
        return;
    }
    kmin = loo_block_red<NT>(kmin, [](U a, U b) { return a < b ? a : b; }, ured);
    kor = loo_block_red<NT>(kor, [](U a, U b) { return a | b; }, ured);
    kand = loo_block_red<NT>(kand, [](U a, U b) { return a & b; }, ured);
    const double a = -(double)K::from(kmin);

    // 2: the key of the (M + 1)-th smallest l
    double c = inf;  // M = 0: nothing is above the cutoff
    if (M > 0) {
        const U diff = kor ^ kand;
        int hi = diff ? K::BITS - (sizeof(U) == 8 ? __builtin_clzll((unsigned long long)diff) : __builtin_clz((unsigned)diff)) : 0;
        U prefix = hi >= K::BITS ? U(0) : (kand >> hi) << hi;  // the bits every key has in common
        unsigned rank = (unsigned)M;
        while (hi > 0) {
            const int lo = hi > kLooDigit ? hi - kLooDigit : 0;
            const unsigned mask = (1u << (hi - lo)) - 1u;
#pragma unroll
            for (int b = 0; b < BPT; ++b) hist[tid * BPT + b] = 0u;
            __syncthreads();
            for (int s = tid; s < S; s += NT) {
                const U k = K::of(row[s]);
                const U above = hi >= K::BITS ? U(0) : ((k ^ prefix) >> hi);
                if (above == U(0)) atomicAdd(hist + ((unsigned)(k >> lo) & mask), 1u);
            }
            __syncthreads();
            unsigned mine = 0;
#pragma unroll
            for (int b = 0; b < BPT; ++b) mine += hist[tid * BPT + b];
            unsigned incl = mine;  // inclusive scan over the lanes: inside the wave, then the waves before this one
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            unsigned before = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) before += w < wave ? wtot[w] : 0u;
            incl += before;
            unsigned excl = incl - mine;
            if (excl <= rank && rank < incl) {  // exactly one lane: the candidates number more than rank
#pragma unroll
                for (int b = 0; b < BPT; ++b) {
                    const unsigned h = hist[tid * BPT + b];
                    if (excl <= rank && rank < excl + h) {
                        sel[0] = (unsigned)(tid * BPT + b);
                        sel[1] = rank - excl;
                    }
                    excl += h;
                }
            }
            __syncthreads();
            prefix |= (U)sel[0] << lo;
            rank = sel[1];
            hi = lo;
            __syncthreads();
        }
        c = -(double)K::from(prefix) - a;
    }

    // 3: the tail into LDS; the sums over the body and over every draw
    if (tid == 0) ntail = 0u;
    __syncthreads();
    double sb = 0.0, sb2 = 0.0, sl = 0.0;
    for (int s = tid; s < S; s += NT) {
        const double x = (double)row[s];
        const double v = -x - a;
        sl += exp(x);
        if (v > c) {
            const unsigned slot = atomicAdd(&ntail, 1u);
            if (slot < (unsigned)XCAP) tail[slot] = v;
        } else {
            const double e = exp(v);
            sb += e;
            sb2 = __builtin_fma(e, e, sb2);
        }
    }
    __syncthreads();
    const int nt = (int)(ntail < (unsigned)XCAP ? ntail : (unsigned)XCAP);  // (n_t <= M <= XCAP by construction)
    sb = loo_block_sum<NT>(sb, dred);
    sb2 = loo_block_sum<NT>(sb2, dred);
    sl = loo_block_sum<NT>(sl, dred);
    int p2 = 1;
    while (p2 < nt) p2 <<= 1;
    for (int i = nt + tid; i < p2; i += NT) tail[i] = inf;
    __syncthreads();
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < p2; i += NT) {
                const int o = i ^ j;
                if (o > i) {
                    const double u = tail[i], w = tail[o];
                    if ((u > w) == ((i & k) == 0)) {
                        tail[i] = w;
                        tail[o] = u;
                    }
                }
            }
            __syncthreads();
        }
    }

    // 4: the fit
    bool raw = nt <= 4;
    double khat = inf, sigma = 0.0, ec = 0.0;
    if (!raw) {
        const double n = (double)nt;
        ec = exp(c);
        for (int i = tid; i < nt; i += NT) xs[i] = exp(tail[i]) - ec;
        __syncthreads();
        const int m = 30 + (int)__builtin_sqrt(n);  // exact for these integers; floor by the conversion
        const double xn = xs[nt - 1], xq = xs[(int)(n / 4.0 + 0.5) - 1];
        if (tid < m) th[tid] = 1.0 / xn + (1.0 - __builtin_sqrt((double)m / ((double)(tid + 1) - 0.5))) / (3.0 * xq);
        __syncthreads();
        for (int j = wave; j < m; j += NW) {
            const double t = th[j];
            double acc = 0.0;
            for (int i = lane; i < nt; i += 64) acc += log1p(-t * xs[i]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) {
                const double kj = acc / n;
                kk[j] = kj;
                LL[j] = n * (log(-t / kj) - kj - 1.0);
            }
        }
        __syncthreads();
        double tw = 0.0;
        if (tid < m) {
            const double Lj = LL[tid];
            double sum = 0.0;
            for (int i = 0; i < m; ++i) sum += exp(LL[i] - Lj);
            tw = th[tid] * (1.0 / sum);
        }
        __syncthreads();
        if (tid < m) kk[tid] = tw;
        __syncthreads();
        double theta = 0.0;
        for (int j = 0; j < m; ++j) theta += kk[j];
        double acc = 0.0;
        for (int i = tid; i < nt; i += NT) acc += log1p(-theta * xs[i]);
        const double k0 = loo_block_sum<NT>(acc, dred) / n;
        sigma = -k0 / theta;
        khat = (n * k0 + 5.0) / (n + 10.0);
        if (!(__builtin_fabs(khat) < inf) || !(__builtin_fabs(sigma) < inf)) {
            raw = true;
            khat = inf;
        }
    }

    // 5: the tail's weights and the closed-form sums
    double tn = 0.0, tw = 0.0, tw2 = 0.0;
    for (int j = tid; j < nt; j += NT) {
        const double v = tail[j];
        double w;
        if (raw) {
            w = exp(v);
        } else {
            const double p = ((double)(j + 1) - 0.5) / (double)nt;
            const double lp = log1p(-p);
            const double q = khat == 0.0 ? -sigma * lp : sigma / khat * (exp(-khat * lp) - 1.0);
            const double wq = ec + q;
            w = wq < 1.0 ? wq : 1.0;
            tn += exp(log(w) - v);
        }
        tw += w;
        tw2 = __builtin_fma(w, w, tw2);
    }
    tn = loo_block_sum<NT>(tn, dred);
    tw = loo_block_sum<NT>(tw, dred);
    tw2 = loo_block_sum<NT>(tw2, dred);
    if (tid == 0) {
        const double num = raw ? (double)S : (double)(S - nt) + tn;
        const double den = sb + tw, den2 = sb2 + tw2;
        out[0] = (log(num) - log(den)) - a;
        out[r] = khat;
        out[2 * r] = den * den / den2;
        out[3 * r] = log(sl / (double)S);
        out[4 * r] = (double)nt;
    }
}

}  // namespace lr
