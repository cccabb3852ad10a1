/*
 * logreg_hip_predict.h -- what to do with the posterior draws of liblogreg_hip.so without taking them off the device: a streaming
 * accumulator of the posterior predictive probability of new rows and of the pointwise log predictive density of labelled rows
 * (lppd and WAIC: Watanabe 2010; Gelman, Hwang & Vehtari 2014; Vehtari, Gelman & Gabry 2017).
 *
 * Draws go in, in any number of batches, from host or device memory; a fixed-size table of per-row statistics comes out.  For
 * prediction rows x_i (i < r), optional labels y_i in {0,1} and draws beta_s (s < S):
 *     eta = x_i . beta_s      pi = sigma(eta)      t = (2 y_i - 1) eta      L = sigma(t)      l = log sigma(t)
 * with  l = min(t, 0) - log1p(exp(-|t|)),  the stable form of the model's own log-likelihood (logreg_hip.h, lr_eval).
 *
 * The table has LR_PRED_ROWS = 5 float64 rows of length r:
 *     row 0   mean over s of pi          the predictive probability P(y = 1 | x_i, data)
 *     row 1   sum  over s of (pi - mean)^2       posterior sd of the probability = sqrt(row 1 / (S - 1))
 *     row 2   mean over s of L           lppd_i = log(row 2)
 *     row 3   mean over s of l
 *     row 4   sum  over s of (l - mean)^2        p_waic,i = row 4 / (S - 1)
 * Rows 2 - 4 are NaN when the accumulator has no labels.  Row 2 is kept beside row 0 on purpose: 1 - mean(pi) loses the small
 * likelihoods that decide lppd.
 *
 * Arithmetic.  Per (draw, row) pair everything is computed in the model's dtype; every sum over draws, the merge of batches and the
 * table are float64.  L <= 1, so the mean of L needs no max-shifted log-sum-exp: a sum of S values in [0, 1] cannot overflow, and it
 * loses nothing unless L itself underflows, which in float64 needs t < -708 (|eta| beyond about 708; about 87 in a float32 model's
 * per-pair arithmetic), far outside any posterior this model can have.  Moments are merged by the pairwise rule of Chan, Golub &
 * LeVeque (1983) in a fixed order and without atomics: the same sequence of calls gives the same bytes.
 *
 * Non-finite input: a draw with a NaN coordinate makes every entry of the table NaN (until lr_predict_reset), never a finite wrong number.
 *
 * A header of its own, as logreg_hip_nuts.h: logreg_hip.h's symbol set is pinned by the test double of the whole ABI; the entry
 * points below are bound from their own table (logreg_amd/_lib.py PREDICT_SYMBOLS).  Status codes, lr_last_error and the pointer
 * conventions are those of logreg_hip.h.  An accumulator reads its model's rows: it may be DESTROYED after the model, but not used; like
 * the model handle it is not thread-safe.
 */
#ifndef LOGREG_HIP_PREDICT_H
#define LOGREG_HIP_PREDICT_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_PRED_ROWS 5

typedef struct lr_predict lr_predict;

/*
 * X_new  [r,p] host doubles (rounded to the model's dtype), or NULL = the model's own design and labels, which are resident
 *        already: then r must be the model's n and y_new must be NULL.
 * y_new  [r] host doubles in {0,1}, or NULL = no labels (rows 2 - 4 of the table are NaN).
 * Errors (with a reason): NULL model / out, r <= 0, r != n with X_new = NULL, non-finite X_new, labels outside {0,1}.
 */
LR_API int lr_predict_create(lr_model* m, const double* X_new, const double* y_new, int64_t r, lr_predict** out);

/*
 * Fold S draws into the accumulator.  draws [S,p] in the model's dtype, host memory (on_device = 0: staged and the call returns
 * when the work is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed once the stream
 * has passed this call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, S <= 0.  (The width of a draw is the model's p by construction: the Python face checks shapes.)
 * Running out of memory leaves the accumulator as it was (the workspaces are sized before anything is folded in).  After a HIP error
 * part-way through a large S the pieces already folded in stay counted: lr_predict_result's n_draws tells, lr_predict_reset clears.
 */
LR_API int lr_predict_accumulate(lr_predict* pp, const void* draws, int64_t S, int32_t on_device, void* stream);

/* table [LR_PRED_ROWS, r] host doubles; n_draws (may be NULL) receives S, the number of draws folded in so far.  Synchronises with
 * the stream of the last accumulate call.  With S = 0 the table is all NaN. */
LR_API int lr_predict_result(lr_predict* pp, double* table, int64_t* n_draws);

/* Forget every draw (S = 0).  The rows and labels stay. */
LR_API int lr_predict_reset(lr_predict* pp);

LR_API void lr_predict_destroy(lr_predict* pp);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_PREDICT_H */
