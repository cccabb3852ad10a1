// lr_rank_math.h -- the scalar arithmetic of include/logreg_hip_rank.h that the device, the host and the CPU double of the tests
// (tests/host/lr_cpu_twin_rank.c) share: the order-preserving integer key of a double, the inverse normal CDF of the z-scale, and the
// float64 finish of the small tables (steps 5 and 6 of the header).  Plain C99 / C++: no HIP type, nothing but <math.h> and <stdint.h>.
#ifndef LR_RANK_MATH_H
#define LR_RANK_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LR_RANK_HD __host__ __device__ static inline
#else
#define LR_RANK_HD static inline
#endif

// rows of the per-series table the device hands to lr_rank_series: sum over m of (mean_m - mean_0), of its square, of acov_m(l), l = 0..L
#define LR_RANK_TAB_HEAD 2

// x -> an unsigned key with key(x) < key(y) <=> x < y for every pair of non-NaN doubles, -0.0 mapped to +0.0 first (they tie);
// -NaN < -inf and +inf < +NaN, so the non-finite values sit at the two ends of a sorted array.
LR_RANK_HD uint64_t lr_rank_key(double x) {
    uint64_t b;
    if (x == 0.0) x = 0.0;
    memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

LR_RANK_HD double lr_rank_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

#define LR_RANK_KEY_NEG_INF 0x000FFFFFFFFFFFFFull /* lr_rank_key(-inf): keys <= it are -inf and the negative NaNs */
#define LR_RANK_KEY_POS_INF 0xFFF0000000000000ull /* lr_rank_key(+inf): keys >= it are +inf and the positive NaNs */
#define LR_RANK_KEY_PAD 0xFFFFFFFFFFFFFFFFull     /* the largest key: what a sorted array is padded with */

// Phi^-1(p), 0 < p < 1: Wichura (1988), Algorithm AS 241, PPND16 (about 1e-16 relative).  Horner, every step an fma.
LR_RANK_HD double lr_rank_ndtri(double p) {
    const double q = p - 0.5;
    double r, num, den;
    if (fabs(q) <= 0.425) {
        r = 0.180625 - q * q;
        num = 2.5090809287301226727e3;
        num = fma(num, r, 3.3430575583588128105e4);
        num = fma(num, r, 6.7265770927008700853e4);
        num = fma(num, r, 4.5921953931549871457e4);
        num = fma(num, r, 1.3731693765509461125e4);
        num = fma(num, r, 1.9715909503065514427e3);
        num = fma(num, r, 1.3314166789178437745e2);
        num = fma(num, r, 3.3871328727963666080);
        den = 5.2264952788528545610e3;
        den = fma(den, r, 2.8729085735721942674e4);
        den = fma(den, r, 3.9307895800092710610e4);
        den = fma(den, r, 2.1213794301586595867e4);
        den = fma(den, r, 5.3941960214247511077e3);
        den = fma(den, r, 6.8718700749205790830e2);
        den = fma(den, r, 4.2313330701600911252e1);
        den = fma(den, r, 1.0);
        return q * num / den;
    }
    r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    if (r <= 5.0) {
        r -= 1.6;
        num = 7.74545014278341407640e-4;
        num = fma(num, r, 2.27238449892691845833e-2);
        num = fma(num, r, 2.41780725177450611770e-1);
        num = fma(num, r, 1.27045825245236838258);
        num = fma(num, r, 3.64784832476320460504);
        num = fma(num, r, 5.76949722146069140550);
        num = fma(num, r, 4.63033784615654529590);
        num = fma(num, r, 1.42343711074968357734);
        den = 1.05075007164441684324e-9;
        den = fma(den, r, 5.47593808499534494600e-4);
        den = fma(den, r, 1.51986665636164571966e-2);
        den = fma(den, r, 1.48103976427480074590e-1);
        den = fma(den, r, 6.89767334985100004550e-1);
        den = fma(den, r, 1.67638483018380384940);
        den = fma(den, r, 2.05319162663775882187);
        den = fma(den, r, 1.0);
    } else {
        r -= 5.0;
        num = 2.01033439929228813265e-7;
        num = fma(num, r, 2.71155556874348757815e-5);
        num = fma(num, r, 1.24266094738807843860e-3);
        num = fma(num, r, 2.65321895265761230930e-2);
        num = fma(num, r, 2.96560571828504891230e-1);
        num = fma(num, r, 1.78482653991729133580);
        num = fma(num, r, 5.46378491116411436990);
        num = fma(num, r, 6.65790464350110377720);
        den = 2.04426310338993978564e-15;
        den = fma(den, r, 1.42151175831644588870e-7);
        den = fma(den, r, 1.84631831751005468180e-5);
        den = fma(den, r, 7.86869131145613259100e-4);
        den = fma(den, r, 1.48753612908506148525e-2);
        den = fma(den, r, 1.36929880922735805310e-1);
        den = fma(den, r, 5.99832206555887937690e-1);
        den = fma(den, r, 1.0);
    }
    const double v = num / den;
    return q < 0.0 ? -v : v;
}

// z-scale of the doubled average rank 2r among S values (step 2)
LR_RANK_HD double lr_rank_z(int64_t twice_r, int64_t S) { return lr_rank_ndtri(((double)twice_r * 0.5 - 0.375) / ((double)S + 0.25)); }

// Steps 5 and 6 on one series' table tab [LR_RANK_TAB_HEAD + L + 1] of M split chains of h values, L = min(max_lag, h - 1) lags (with_ess
// == 0: L = 0, the R-hat alone).  out: rhat, ess, capped (0 / 1), pairs kept; NaN where the header says so.
static inline void lr_rank_series(const double* tab, int64_t h, int64_t M, int L, int max_lag, int with_ess, double* rhat, double* ess, double* capped,
                                  double* pairs) {
    const double hd = (double)h, Md = (double)M, S = hd * Md;
    const double W = tab[LR_RANK_TAB_HEAD] / Md * hd / (hd - 1.0);
    const double B = (tab[1] - tab[0] * tab[0] / Md) / (Md - 1.0);
    const double V = (hd - 1.0) / hd * W + B;
    *rhat = *ess = *capped = *pairs = (double)NAN;
    if (h < 2 || !(W > 0.0) || !isfinite(W) || !isfinite(V)) return;
    *rhat = sqrt(V / W);
    if (!with_ess) return;
    const int npairs = (L + 1) / 2;
    double sum = 0.0, prev = 0.0, last = 0.0;
    int k = 0, stopped = 0;
    for (; k < npairs; ++k) {
        const double r0 = k == 0 ? 1.0 : 1.0 - (W - tab[LR_RANK_TAB_HEAD + 2 * k] / Md) / V;
        const double r1 = 1.0 - (W - tab[LR_RANK_TAB_HEAD + 2 * k + 1] / Md) / V;
        double P = r0 + r1;
        if (!(P > 0.0)) {
            stopped = 1;
            last = r0 > 0.0 ? r0 : 0.0;
            break;
        }
        if (k > 0 && P > prev) P = prev;
        sum += P;
        prev = P;
    }
    double tau = -1.0 + 2.0 * sum + last;
    const double floor_tau = 1.0 / log10(S);
    if (!(tau >= floor_tau)) tau = floor_tau;
    *ess = S / tau;
    *capped = (!stopped && L == max_lag && h - 1 > max_lag) ? 1.0 : 0.0;
    *pairs = (double)k;
}

#endif  // LR_RANK_MATH_H
