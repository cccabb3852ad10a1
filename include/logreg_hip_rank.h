/*
 * logreg_hip_rank.h -- rank-normalised split-R-hat with bulk and tail effective sample sizes (Vehtari, Gelman, Simpson, Carpenter &
 * Buerkner 2021) of the kept draws of liblogreg_hip.so, without taking them off the device.  Unlike the other accumulators this one is
 * not a sum over draws: ranks need a global order of every coordinate's draws, so the accumulator STORES the blocks [k, C, p] it is fed
 * (device memory, time order, max_steps steps at the most) and sorts them when a result is asked for.
 *
 * Definition.  Everything below is float64 whatever the dtype of the draws.  With n steps stored, h = n / 2 (integer division); the
 * series used are steps [0, h) and [h, 2h) of every chain (an odd last step is ignored, as logreg_amd.diagnostics.split_rhat does):
 * M = 2C split chains of h values, S = 2hC values per coordinate.  Split chain m = 2c + (t >= h).  Per coordinate:
 *   1. Ranks.  The draws are widened exactly to float64 and compared as IEEE numbers (-0.0 ties with +0.0).  With lo = #{y < x} and
 *      hi = #{y <= x} over the S values, the average rank is r = (lo + hi + 1) / 2; 2r is an exact integer.
 *   2. z-scale.  z = Phi^-1((r - 3/8) / (S + 1/4)), Phi^-1 by Wichura's AS 241 (PPND16).
 *   3. Fold.  med = (x_(S/2) + x_(S/2+1)) / 2 (order statistics, 1-based), f = |x - med|, zf = the z-scale of f (ranked by float64
 *      equality).
 *   4. Tail indicators.  q05 = the order statistic with 0-based index (S - 1) / 20, q95 = the one with 0-based index 19 (S - 1) / 20
 *      (integer divisions: type-7 quantiles without the interpolation, which cannot change an indicator).  I05 = [x <= q05],
 *      I95 = [x <= q95], as 0.0 / 1.0.
 *   5. Per series v [h, M] (z, zf, I05, I95), per split chain m:  d_t = v_t - v_0 (the pivot),  dbar = (sum_t d_t) / h,
 *      mean_m = v_0 + dbar,  e_t = d_t - dbar,  acov_m(l) = (1/h) sum_{t < h-l} e_t e_{t+l}  for l <= L = min(max_lag, h - 1)
 *      (a constant chain has acov_m exactly 0).
 *          W = (mean over m of acov_m(0)) h / (h - 1)          B = the ddof-1 variance of the mean_m (pivoted at mean_0 before squaring)
 *          V = (h - 1) / h  W + B                               rhat(v) = sqrt(V / W)
 *      rhat_bulk = rhat(z), rhat_tail = rhat(zf), rhat = the larger of the two.
 *   6. ess(v).  rho_l = 1 - (W - mean over m of acov_m(l)) / V, rho_0 = 1.  Pairs P_j = rho_2j + rho_2j+1 for 2j + 1 <= L, kept up to
 *      the first P_k that is not > 0 and made non-increasing (P_j = min(P_j, P_j-1)).  tau = -1 + 2 sum_{j<k} P_j + max(rho_2k, 0), the
 *      last term (Stan's) only when a non-positive pair ended the scan.  tau is floored at 1 / log10(S); ESS = S / tau.  If the lags
 *      run out at max_lag before a non-positive pair while h - 1 > max_lag, the figure uses every pair and the series is flagged
 *      CAPPED (the convention of logreg_hip_acf.h).  ess_bulk = ess(z); ess_tail = min(ess(I05), ess(I95)).
 *      This is the estimator of R's `posterior` package (ess_bulk, ess_tail, rhat) except for the lag cap and the end-of-series bound
 *      (posterior follows the autocovariance to lag h - 1 through an FFT and stops three lags before the end).
 *   7. Edge cases.  A coordinate that holds a NaN or an infinity among its S used values gets NaN in every float row, and the number
 *      of such values in row 11; the other coordinates are not touched by it.  W = 0 (a constant coordinate, or one whose z or
 *      indicators are constant) gives NaN for what is derived from that series.  n < 4 gives NaN in every float row (nothing is
 *      sorted; row 11 is 0).  Never a finite wrong number.
 *
 * Result table: LR_RANK_ROWS float64 rows of length p.
 *     0 rhat_bulk   1 rhat_tail   2 rhat   3 ess_bulk   4 ess_tail   5 / 6 / 7 capped (0 / 1) of ess(z), ess(I05), ess(I95)
 *     8 median (= med)   9 q05   10 q95 (exact order statistics)   11 n_nonfinite   12 / 13 / 14 pairs kept (k) of ess(z), ess(I05), ess(I95)
 *
 * Arithmetic on the device: the order comes from a bitonic sort of order-preserving 64-bit integer keys (no payload, no atomics), lo
 * and hi from two binary searches per draw; the lag sums are one fma per (t, l) in t order, the chains are summed over a fixed tree,
 * and the small tables are finished on the host in float64.  Draws are stored, so the same draws give the same bytes however they were
 * cut into calls.
 *
 * A header of its own, as logreg_hip_acf.h: logreg_hip.h's symbol set is pinned; the entry points below are bound from their own table
 * (logreg_amd/_lib.py RANK_SYMBOLS).  Status codes, lr_last_error and the pointer and stream conventions are those of logreg_hip.h /
 * logreg_hip_acf.h.  An accumulator is not thread-safe.
 */
#ifndef LOGREG_HIP_RANK_H
#define LOGREG_HIP_RANK_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_RANK_MAX_LAG 255
#define LR_RANK_MAX_DRAWS (1ll << 24) /* draws per coordinate, C * max_steps */
#define LR_RANK_ROWS 15

typedef struct lr_rank lr_rank;

/*
 * C chains x p coordinates of draws of `dtype` (LR_F32 / LR_F64) on `device`, room for max_steps time steps; max_lag odd, 1 <= max_lag
 * <= LR_RANK_MAX_LAG.  Errors (with a reason): NULL out, C, p or max_steps <= 0, max_lag even or out of range, a bad dtype
 * (LR_ERR_INVALID); C * max_steps > LR_RANK_MAX_DRAWS (LR_ERR_UNSUPPORTED); out of memory.
 */
LR_API int lr_rank_create(int device, int32_t dtype, int64_t C, int32_t p, int64_t max_steps, int32_t max_lag, lr_rank** out);

/*
 * Store k more time steps.  block [k, C, p] in the accumulator's dtype, rows in time order, host memory (on_device = 0: the call
 * returns when the copy is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed once the
 * stream has passed this call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, k <= 0, more than max_steps steps in all, out of memory -- each leaves the accumulator as it was.
 */
LR_API int lr_rank_accumulate(lr_rank* r, const void* block, int64_t k, int32_t on_device, void* stream);

/*
 * table [LR_RANK_ROWS, p] host doubles; n_draws (may be NULL) receives n, the steps stored.  Synchronises with the stream of the last
 * accumulate call; the stored draws are not changed (more may follow).  Every workspace is grown before anything is enqueued.
 */
LR_API int lr_rank_result(lr_rank* r, double* table, int64_t* n_draws);

/*
 * The ranks of coordinate j (0 <= j < p): twice_r [2h, C] host int64 receives 2r of every used draw (folded != 0: of f), z [2h, C] host
 * doubles or NULL its z-scale; n_used (may be NULL) receives 2h.  With n < 2 nothing is written.  What a rank histogram per chain is
 * drawn from; the state is not changed.
 */
LR_API int lr_rank_ranks(lr_rank* r, int32_t j, int32_t folded, int64_t* twice_r, double* z, int64_t* n_used);

/* Forget every draw (n = 0). */
LR_API int lr_rank_reset(lr_rank* r);

LR_API void lr_rank_destroy(lr_rank* r);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_RANK_H */
