/*
 * logreg_hip_acf.h -- autocorrelation and Geyer's effective sample size of the kept draws of liblogreg_hip.so, without taking them
 * off the device: a streaming accumulator that needs no model, only blocks [k, C, p] of draws in time order (any sampler's, NUTS
 * included).  It is the estimator of logreg_amd.diagnostics.ess_geyer (Geyer 1992, initial positive sequence), restricted to the
 * first K lags, for every series (chain c, coordinate j) at once -- what smfsb::mcmcSummary reports and plots in the reference's
 * Python/analyse.R:17-19, for 65 536 chains as for one.
 *
 * Definition, per series of n values x_t (m = their mean):
 *     acov[l] = (1/n) sum_{t < n-l} (x_t - m)(x_{t+l} - m)     (biased, globally centred; 0 for l >= n)      rho = acov / acov[0]
 *     Gamma_j = rho[2j] + rho[2j+1]   for j < min((K+1)/2, n/2),   truncated at the first Gamma_j <= 0
 *     tau = -1 + 2 sum of the kept Gamma_j        ESS = n / tau        (ESS = n when n < 4, acov[0] <= 0 or tau <= 0)
 * A series whose scan ends at (K+1)/2 pairs without meeting a Gamma_j <= 0 while n/2 would have allowed more is CAPPED: its ESS uses
 * all (K+1)/2 pairs, and it is counted.
 *
 * The table `sums` has LR_ACF_ROWS(K) = K + 4 float64 rows of length p, every entry a sum over the chains (tables of chain shards add):
 *     row 0        sum over c of ESS_c           (= diagnostics.ess_pooled(samples, max_chains=None) where no series is capped)
 *     row 1        number of capped chains
 *     row 2        number of chains whose ESS is NaN
 *     row 3 + l    sum over c of acov_c[l],  l = 0 .. K
 * The sums over chains run over a fixed tree, without atomics: the same sequence of calls gives the same bytes.
 *
 * Non-finite input: a series that holds a NaN or an inf gets NaN for its ESS and its acov (rows 0 and 3.. of its coordinate become
 * NaN, row 2 counts it), never a finite wrong number.
 *
 * Arithmetic.  Everything is float64 whatever the dtype of the draws.  A series is pivoted at its own first value,
 * xs_t = x_t - x_0 (so a posterior far from 0 costs no digits), and its state is the lag sums S_l = sum_t xs_t xs_{t-l} (l = 0..K, one
 * fma per (t, l) in t order: the result does not depend on how the draws were cut into calls), the total sum of xs, the first K and
 * the last K values, about 8 (3K + 3) bytes per series.  At result time, with ms = total / n,
 *     acov[l] = (S_l - ms (H_l + T_l) + (n - l) ms^2) / n,    H_l = total - (sum of the last l values),  T_l = total - (sum of the first l).
 *
 * A header of its own, as logreg_hip_nuts.h and logreg_hip_predict.h: logreg_hip.h's symbol set is pinned; the entry points below are
 * bound from their own table (logreg_amd/_lib.py ACF_SYMBOLS).  Status codes, lr_last_error and the pointer and stream conventions
 * are those of logreg_hip.h / logreg_hip_predict.h.  An accumulator is not thread-safe.
 */
#ifndef LOGREG_HIP_ACF_H
#define LOGREG_HIP_ACF_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_ACF_MAX_LAG 255
#define LR_ACF_ROWS(K) ((K) + 4)

typedef struct lr_acf lr_acf;

/*
 * C chains x p coordinates of draws of `dtype` (LR_F32 / LR_F64) on `device`; max_lag = K odd, 1 <= K <= LR_ACF_MAX_LAG (lags 0..K
 * are (K+1)/2 Geyer pairs).  Errors (with a reason): NULL out, C or p <= 0, K even or out of range, a bad dtype, out of memory.
 */
LR_API int lr_acf_create(int device, int32_t dtype, int64_t C, int32_t p, int32_t max_lag, lr_acf** out);

/*
 * Fold k more time steps in.  block [k, C, p] in the accumulator's dtype, rows in time order, host memory (on_device = 0: staged, and
 * the call returns when the work is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed
 * once the stream has passed this call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, k <= 0, out of memory -- which leaves the accumulator as it was (the staging buffer is sized before
 * anything is folded in).
 */
LR_API int lr_acf_accumulate(lr_acf* acf, const void* block, int64_t k, int32_t on_device, void* stream);

/*
 * sums [LR_ACF_ROWS(K), p] host doubles; ess_chain [C, p] host doubles or NULL (the per-series ESS); n_draws (may be NULL) receives
 * n, the time steps folded in so far.  Synchronises with the stream of the last accumulate call; the state is not changed (more
 * draws may follow).  With n = 0 every entry is NaN.
 */
LR_API int lr_acf_result(lr_acf* acf, double* sums, double* ess_chain, int64_t* n_draws);

/* Forget every draw (n = 0). */
LR_API int lr_acf_reset(lr_acf* acf);

LR_API void lr_acf_destroy(lr_acf* acf);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_ACF_H */
