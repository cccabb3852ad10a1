/*
 * logreg_hip_marginals.h -- the shape of the posterior marginals of the kept draws of liblogreg_hip.so, without taking them off the
 * device: a streaming accumulator that needs no model, only blocks [k, C, p] of draws in time order (any sampler's).  Per coordinate j,
 * pooled over chains and time, it keeps a histogram on a fixed grid, the smallest and the largest draw, and the first four power sums:
 * what scipy.stats.describe prints at the end of the reference's Python/fit-np-hmc.py:113-117 (nobs, min/max, mean, variance, skewness,
 * kurtosis) and what smfsb::mcmcSummary prints and draws in Python/analyse.R (quartiles, a histogram per coordinate) -- for 65 536
 * chains as for one.  Quantiles, equal-tailed and shortest intervals and densities are read off the histogram on the host
 * (logreg_amd/marginals.py).
 *
 * Definitions.  Every draw x is first converted to double.  B = bins; lo_j < hi_j is the grid of coordinate j.
 *
 * Bin.     invw_j = B / (hi_j - lo_j), computed once on the host in float64.       t = (x - lo_j) * invw_j
 *          (one subtraction, then one multiplication: nothing here can contract to an fma).  The column of x among the
 *          LR_MARG_COLS(B) = B + 3 columns of its coordinate:
 *              x is NaN           -> B + 2
 *              t <  0             -> 0          (underflow: exactly the draws x < lo_j; -inf too)
 *              t >= B or x >= hi  -> B + 1      (overflow; x == hi_j and +inf too.  The product can round (hi_j - lo_j) * invw_j to
 *                                                just below B, so the comparison with hi_j itself is part of the rule)
 *              otherwise          -> 1 + (int)floor(t)                 (x == lo_j is bin 0)
 *          counts [p, B + 3] are uint64 and exact: integers, so they do not depend on summation order, on how the draws were cut into
 *          calls, on build flags or on how workgroups interleave.
 *
 * min/max. (table rows 0 and 1) over the non-NaN draws, exact: np.nanmin / np.nanmax of the dtype-rounded input; NaN when a
 *          coordinate has no non-NaN draw.
 *
 * Power sums (table rows 2..5).  c_j = (lo_j + hi_j) / 2, s_j = 2 / (hi_j - lo_j), u = (x - c_j) * s_j (in [-1, 1] inside the grid: a
 *          posterior far from 0 costs no digits) and S_k = sum u^k, k = 1..4.  Per series (chain, coordinate), in time order:
 *              S1 += u        S2 = fma(u, u, S2)        S3 = fma(u*u, u, S3)        S4 = fma(u*u, u*u, S4)
 *          (u*u one rounded product).  The per-series sums are persistent state; at result time they are summed over the chains by a
 *          fixed tree, without atomics: the same draws give the same bytes however they are cut into calls, and in every build.
 *          A NaN or an inf among a coordinate's draws makes its rows 2..5 non-finite, never a finite wrong number.
 *
 * With n = 0 draws the counts are 0 and the table is NaN.
 *
 * A header of its own, as logreg_hip_acf.h: logreg_hip.h's symbol set is pinned; the entry points below are bound from their own table
 * (logreg_amd/_lib.py MARG_SYMBOLS).  Status codes, lr_last_error and the pointer and stream conventions are those of logreg_hip.h /
 * logreg_hip_acf.h.  An accumulator is not thread-safe.
 */
#ifndef LOGREG_HIP_MARGINALS_H
#define LOGREG_HIP_MARGINALS_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_MARG_MAX_BINS 1024
#define LR_MARG_COLS(B) ((B) + 3)
#define LR_MARG_ROWS 6

typedef struct lr_marg lr_marg;

/*
 * C chains x p coordinates of draws of `dtype` (LR_F32 / LR_F64) on `device`; bins in 1..LR_MARG_MAX_BINS; lo [p], hi [p] host doubles,
 * finite, lo < hi.  Errors (with a reason): NULL out / lo / hi, C or p <= 0, bins out of range, a bad dtype, a bad grid, out of memory.
 */
LR_API int lr_marg_create(int device, int32_t dtype, int64_t C, int32_t p, int32_t bins, const double* lo, const double* hi, lr_marg** out);

/*
 * Fold k more time steps in.  block [k, C, p] in the accumulator's dtype, rows in time order, host memory (on_device = 0: staged, and
 * the call returns when the work is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed
 * once the stream has passed this call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, k <= 0, out of memory -- which leaves the accumulator as it was (the staging buffer is sized before
 * anything is folded in).
 */
LR_API int lr_marg_accumulate(lr_marg* m, const void* block, int64_t k, int32_t on_device, void* stream);

/*
 * counts [p, LR_MARG_COLS(bins)] host uint64; table [LR_MARG_ROWS, p] host doubles (min, max, S1, S2, S3, S4); either may be NULL;
 * n_draws (may be NULL) receives n, the time steps folded in so far.  Synchronises with the stream of the last accumulate call; the
 * state is not changed (more draws may follow).
 */
LR_API int lr_marg_result(lr_marg* m, uint64_t* counts, double* table, int64_t* n_draws);

/* Forget every draw (n = 0); the grid stays. */
LR_API int lr_marg_reset(lr_marg* m);

LR_API void lr_marg_destroy(lr_marg* m);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_MARGINALS_H */
