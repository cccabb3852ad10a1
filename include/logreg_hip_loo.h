/*
 * logreg_hip_loo.h -- Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO) of liblogreg_hip.so from draws
 * that stay on the device: elpd_loo per observation with its diagnostic, the Pareto shape k-hat (Vehtari, Gelman & Gabry 2017;
 * Vehtari, Simpson, Gelman, Yao & Gabry 2024; the generalised-Pareto fit of Zhang & Stephens 2009 as the `loo` package and arviz use it).
 *
 * Two stages.
 *   fill   lr_loo_accumulate appends draws beta_s to the accumulator's matrix of pointwise log-likelihoods of the model's OWN rows,
 *              l[s, i] = min(t, 0) - log1p(exp(-|t|)),   t = (2 y_i - 1) x_i . beta_s,
 *          computed per pair in the model's dtype exactly as lr_predict_accumulate computes its l (logreg_hip_predict.h).
 *   PSIS   lr_loo_result (or lr_psis on a caller's matrix) works on one observation at a time, on l_s (s < S) widened exactly to float64:
 *            a = max_s(-l_s), v_s = -l_s - a (<= 0): the shifted log importance ratios.
 *            M = min(floor(S / 5), m3), m3 the smallest integer with m3^2 >= 9 S.  M = 0: no tail.  Else c = the (S - M)-th smallest v
 *            and the tail is {s : v_s > c}, STRICTLY greater, of size n_t <= M (ties at the cutoff shrink it).
 *            n_t <= 4: khat = +inf and the weights stay raw, w_s = exp(v_s).
 *            n_t >= 5: the tail sorted ascending v_(1..n_t), x_j = exp(v_(j)) - exp(c), n = n_t, m = 30 + floor(sqrt(n)),
 *                theta_j = 1 / x_n + (1 - sqrt(m / (j - 0.5))) / (3 x_q), q = floor(n / 4 + 0.5) (1-based), j = 1..m
 *                k_j = mean_i log1p(-theta_j x_i)      L_j = n (log(-theta_j / k_j) - k_j - 1)      omega_j = 1 / sum_i exp(L_i - L_j)
 *                theta = sum_j theta_j omega_j         k = mean_i log1p(-theta x_i)     sigma = -k / theta     k <- (n k + 5) / (n + 10)
 *              k or sigma not finite: khat = +inf, raw weights.  Otherwise khat = k and the tail weights are replaced by
 *                w_j = min(exp(c) + sigma / k (exp(-k log1p(-p_j)) - 1), 1),  p_j = (j - 0.5) / n_t   (k = 0: -sigma log1p(-p_j))
 *              -- always, whatever k is; the truncation is at the largest raw weight (1 after the shift).
 *            Every draw outside the tail has weight x likelihood = e^-a, so with the sums over the body B and the tail:
 *                elpd_i  = log((S - n_t) + sum_j exp(log w_j - v_(j))) - log(sum_B exp(v_s) + sum_j w_j) - a
 *                n_eff_i = (sum w)^2 / sum w^2           lppd_i = log((1 / S) sum_s exp(l_s))
 *            (raw weights: the first bracket is S).  r_eff = 1: no correction for the autocorrelation of the draws.
 *            A limit of n_eff as defined: both sums are plain float64, so where every smoothed weight lies below about 1e-162 the sum
 *            of squares underflows to 0 and n_eff_i is 0 / 0 = NaN from a finite column, while elpd_i, khat_i and lppd_i stay finite.
 *            It takes a fitted tail of tiny scale under a cutoff of exp(-thousands) -- log-likelihoods spread over thousands of nats,
 *            khat far above 0.7, which flags the observation anyway (tests/test_predict_regimes_cpu.py reaches it).
 *
 * The table has LR_LOO_ROWS = 5 float64 rows of length n:  elpd_loo_i, khat_i, n_eff_i, lppd_i, n_tail_i.
 *
 * Non-finite input: an observation whose column holds a NaN (or an infinity) gets five NaNs, never a finite wrong number; the other
 * observations of an lr_psis matrix are unaffected.  Through the model a NaN coordinate in a draw reaches every row.
 * Every float64 sum runs over a fixed tree, selection and compaction use integer atomics only: the same matrix gives the same bytes.
 * The tail lives in on-chip memory: at most LR_LOO_MAX_DRAWS draws per observation (M <= 3072).
 *
 * A header of its own, as logreg_hip_predict.h: logreg_hip.h's symbol set is pinned by the test double of the whole ABI; the entry
 * points below are bound from their own table (logreg_amd/_lib.py LOO_SYMBOLS).  Status codes, lr_last_error and the pointer
 * conventions are those of logreg_hip.h.  An accumulator reads its model's rows: it may be DESTROYED after the model, but not used; like
 * the model handle it is not thread-safe.
 */
#ifndef LOGREG_HIP_LOO_H
#define LOGREG_HIP_LOO_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_LOO_ROWS 5
#define LR_LOO_MAX_DRAWS 1048576

typedef struct lr_loo lr_loo;

/*
 * An accumulator over the model's own n rows and labels with room for max_draws draws: a device buffer of n x max_draws values of
 * the model's dtype.  Errors (with a reason, *out untouched): NULL model / out, max_draws <= 0 (LR_ERR_INVALID), max_draws beyond
 * LR_LOO_MAX_DRAWS (LR_ERR_UNSUPPORTED), allocation failure (LR_ERR_NOMEM).
 */
LR_API int lr_loo_create(lr_model* m, int64_t max_draws, lr_loo** out);

/*
 * Append S draws.  draws [S,p] in the model's dtype, host memory (on_device = 0: staged in pieces, the call returns when the work is
 * done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed once the stream has passed this
 * call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, S <= 0, more than max_draws draws in all -- refused before anything is enqueued, the accumulator as it was.
 */
LR_API int lr_loo_accumulate(lr_loo* acc, const void* draws, int64_t S, int32_t on_device, void* stream);

/* host_out [S, n] in the model's dtype, in arrival order (may be NULL to read the count only); n_draws (may be NULL) receives S. */
LR_API int lr_loo_loglik(lr_loo* acc, void* host_out, int64_t* n_draws);

/* table [LR_LOO_ROWS, n] host doubles from the draws so far; n_draws (may be NULL) receives S.  Synchronises with the stream of the
 * last accumulate call; may be called repeatedly and between accumulate calls.  With S = 0 the table is all NaN. */
LR_API int lr_loo_result(lr_loo* acc, double* table, int64_t* n_draws);

/* Forget every draw (S = 0).  The buffer stays. */
LR_API int lr_loo_reset(lr_loo* acc);

LR_API void lr_loo_destroy(lr_loo* acc);

/*
 * The PSIS stage alone: loglik [S, r] of dtype LR_F32 / LR_F64 from host (on_device = 0) or device memory (on_device = 1, read on
 * `stream`) -> table [LR_LOO_ROWS, r] host doubles; the call returns when the table is written.  Needs no model: gathered shards of
 * a multi-rank run go through this.  Errors: NULL arguments, S <= 0 or r <= 0, a dtype other than the two (LR_ERR_INVALID);
 * S > LR_LOO_MAX_DRAWS (LR_ERR_UNSUPPORTED); allocation failure (LR_ERR_NOMEM).
 */
LR_API int lr_psis(int device, const void* loglik, int64_t S, int64_t r, int32_t dtype, int32_t on_device, double* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_LOO_H */
