/*
 * logreg_hip_bridge.h -- the log marginal likelihood  log p(y) = log INT exp(lpost(beta)) dbeta  of liblogreg_hip.so by bridge sampling
 * from draws that stay on the device: Meng & Wong's (1996) optimal bridge with a Gaussian proposal, as Gronau et al.'s `bridgesampling`
 * runs it, with the relative mean-squared error of Fruehwirth-Schnatter (2004).  lpost carries the normalised prior, constants included,
 * so the integral is p(y) with no correction.
 *
 * Definition.
 *   proposal   g = N(mu, Sigma), Sigma [p][p] symmetric positive definite.  On the host in float64, nothing contracted, sums in ascending
 *              index order: the Cholesky factor  Sigma = L L^T  (L_ij = (Sigma_ij - sum_{k<j} L_ik L_jk) / L_jj, L_ii = sqrt(pivot)) and its
 *              inverse W = L^-1 by forward substitution.  A Sigma with an entry of its lower triangle that is not finite, or a pivot that
 *              is not > 0 and finite, is refused (LR_ERR_INVALID) -- what lr_dense_factor refuses, for every p up to 128.
 *              c_g = -sum_i log L_ii - (p / 2) log(2 pi).
 *   term       l(theta) = lpost(theta) - log g(theta), a float64, of a draw theta [p] AS IT IS STORED in the model's dtype T:
 *                lpost   sum over the rows i < n of l_i = min(t_i, 0) - log1p(exp(-|t_i|)), t_i = xs_i . theta, each l_i computed in T exactly
 *                        as lr_predict_accumulate / lr_loo_accumulate compute theirs (logreg_hip_predict.h; saturated logits included),
 *                        then widened and summed in float64 over a fixed tree:
 *                          rows are cut into slices of 512; in a slice, lane t < 256 adds its rows t, t + 256 in that order, a lane
 *                          without a row adds 0; the 64 lanes of a wave by a xor butterfly (both partners form the same sum), the
 *                          four waves in wave order; the slices in slice order, starting from the first slice's sum;
 *                        plus the prior in float64:  lprior = fma(-0.5, sum_j inv_var_j theta_j^2, lprior_const), the sum by fma in
 *                        ascending j from 0.
 *                log g   in float64:  d_j = theta_j - mu_j;  y_i = sum_{j<=i} W_ij d_j and q = sum_i y_i^2, both by fma in ascending
 *                        order from 0;  log g = fma(-0.5, q, c_g).
 *   posterior terms   l1_i, i < N1: the draws given to lr_bridge_accumulate, in arrival order.
 *   proposal terms    l2_j, j < N2: the terms of theta~_j = mu + L z_j, generated on the device when the accumulator is created.
 *                z_j [p] standard normals from Philox4x32-10, key = seed, counter = (j lo, j hi, 0, LR_BRIDGE_TAG | b): block b gives the
 *                normals 4 b .. 4 b + 3 by Box-Muller exactly as the samplers' normals are made (logreg_hip.h "Random streams"; in the
 *                model's dtype).  The block words used here are 0x08000000 .. 0x0800001F.  That range was free: the samplers'
 *                normal blocks are b < 32, Polya-Gamma's lie in [0x10000000, 0x20000000), NUTS' leaves in [0x20000000, 0x20000100), its
 *                doublings in [0x40000000, 0x40000010), and the accept uniform is 0x80000000 (the list at the top of csrc/lr_device.h,
 *                lr_nuts.h, logreg_hip_pg.h) -- so a proposal shares no counter with any chain even under the same seed.
 *                theta~_ji = mu_i + sum_{k<=i} L_ik z_jk by fma in ascending k from mu_i, in float64, then ROUNDED to T: lpost and log g
 *                are both evaluated at the rounded value.  Draw j depends on (seed, j) alone.
 *   weights    s1 = n_eff / (n_eff + N2), s2 = N2 / (n_eff + N2); n_eff is the caller's (lr_bridge_result; <= 0 or NaN means N1).
 *   iteration  in log space, LAE = logaddexp, LSE = log-sum-exp:
 *                log r <- [LSE_j(l2_j - LAE(log s1 + l2_j, log s2 + log r)) - log N2] - [LSE_i(-LAE(log s1 + l1_i, log s2 + log r)) - log N1]
 *              from log r = LSE_j(l2_j) - log N2, the plain importance-sampling estimate (iteration 0); stopped after the first
 *              iteration whose change is <= tol max(1, |log r|) (converged = 1) or after maxit iterations (converged = 0).
 *              Both bracket terms are monotone in l, so each LSE is shifted by its largest term, found from max l2 / min l1 alone.
 *   error      The estimate is the ratio of mean_j p / (s1 p + s2 g) over the proposal draws to mean_i g / (s1 p + s2 g) over the posterior
 *              draws (p = exp(lpost) / r the normalised posterior), so the delta method needs the spread of exactly these two, as
 *              `bridgesampling` computes it:
 *              f1_j = e^(l2_j - log r) / (s1 e^(l2_j - log r) + s2) = 1 / (s1 + s2 e^(log r - l2_j))   over the PROPOSAL terms,
 *              f2_i = 1 / (s1 e^(l1_i - log r) + s2)                                                   over the POSTERIOR terms.
 *              (The two quotients exchanged -- 1 / (..) over l2 and e^x / (..) over l1 -- are a different number whenever s1 != s2:
 *              s1 e^x / (..) + s2 / (..) = 1 makes their variances proportional, not their relative variances.)
 *              re^2 = var(f1) / (mean(f1)^2 N2) + var(f2) / (mean(f2)^2 n_eff),  var with the divisor N - 1 (0 for N = 1);  se = sqrt(re^2),
 *              the standard error of logml.  Means and variances from shifted sums (pivot: f at max l2 / min l1).
 *   non-finite a term that is NaN or +-inf is never dropped: it is counted, and logml and se are NaN (min / max are over the finite terms).
 * Every float64 sum over the terms runs over a fixed tree for a given (N1, N2): blocks of 4096 terms, lane t of 256 adds its terms
 * t, t + 256, ... in order, butterfly, waves in order; the blocks' partials likewise in a single workgroup.  No float atomics: the same
 * terms give the same bytes, and a term's bytes do not depend on how the draws were cut into calls or pieces, nor on where they lay.
 *
 * The table has LR_BRIDGE_ROWS = 12 float64 entries:
 *   0 logml   1 se   2 iterations   3 converged   4 N1   5 N2   6 n_eff used   7 non-finite terms   8 min l1   9 max l1   10 min l2   11 max l2
 *
 * A header of its own, as logreg_hip_loo.h: logreg_hip.h's symbol set is pinned by the test double of the whole ABI; the entry points
 * below are bound from their own table (logreg_amd/_lib.py BRIDGE_SYMBOLS).  Status codes, lr_last_error and the pointer conventions are
 * those of logreg_hip.h.  An accumulator reads its model's rows: it may be DESTROYED after the model, but not used; like the model
 * handle it is not thread-safe.
 */
#ifndef LOGREG_HIP_BRIDGE_H
#define LOGREG_HIP_BRIDGE_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_BRIDGE_ROWS 12
#define LR_BRIDGE_MAX_DRAWS 1048576
#define LR_BRIDGE_TAG 0x08000000u

typedef struct lr_bridge lr_bridge;

/*
 * An accumulator of up to max_draws posterior terms of the model, with the n_proposal proposal terms computed before the call returns.
 * mu [p], cov [p][p] host doubles.  Errors (with a reason, *out untouched): NULL arguments, max_draws <= 0, n_proposal <= 0, a mu that is
 * not finite, a cov that is refused (LR_ERR_INVALID); max_draws or n_proposal beyond LR_BRIDGE_MAX_DRAWS (LR_ERR_UNSUPPORTED); allocation
 * failure (LR_ERR_NOMEM).
 */
LR_API int lr_bridge_create(lr_model* m, const double* mu, const double* cov, int64_t max_draws, int64_t n_proposal, uint64_t seed, lr_bridge** out);

/*
 * Append the terms of S draws.  draws [S,p] in the model's dtype, host memory (on_device = 0: staged in pieces, the call returns when the
 * work is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed once the stream has passed this
 * call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, S <= 0, more than max_draws draws in all -- refused before anything is enqueued, the accumulator as it was.
 */
LR_API int lr_bridge_accumulate(lr_bridge* acc, const void* draws, int64_t S, int32_t on_device, void* stream);

/* l1 [N1], l2 [N2] host doubles (each may be NULL); n1, n2 (each may be NULL) receive the counts. */
LR_API int lr_bridge_terms(lr_bridge* acc, double* l1, double* l2, int64_t* n1, int64_t* n2);

/* The proposal draws theta~ [N2, p] in the model's dtype, regenerated from (seed, j) (host_out may be NULL); n2 (may be NULL) receives N2. */
LR_API int lr_bridge_proposal(lr_bridge* acc, void* host_out, int64_t* n2);

/* table [LR_BRIDGE_ROWS] host doubles from the terms so far.  Synchronises with the stream of the last accumulate call; may be called
 * repeatedly and between accumulate calls.  With N1 = 0, logml and se are NaN and iterations 0.  Errors: NULL arguments, tol < 0 or NaN,
 * maxit < 0 (LR_ERR_INVALID). */
LR_API int lr_bridge_result(lr_bridge* acc, double n_eff, double tol, int32_t maxit, double* table);

/* Forget every posterior draw (N1 = 0).  The proposal terms stay. */
LR_API int lr_bridge_reset(lr_bridge* acc);

LR_API void lr_bridge_destroy(lr_bridge* acc);

/*
 * The iteration and the error alone on any two vectors of terms: l1 [N1], l2 [N2] float64 from host (on_device = 0) or device memory
 * (on_device = 1, read on `stream`) -> table [LR_BRIDGE_ROWS]; the call returns when the table is written.  Needs no model: gathered
 * shards of a multi-rank run go through this.  The same terms give the bytes of lr_bridge_result.
 * Errors: NULL arguments, N1 <= 0 or N2 <= 0, a bad tol / maxit (LR_ERR_INVALID); N1 or N2 beyond 2^31 - 1 (LR_ERR_UNSUPPORTED).
 */
LR_API int lr_bridge_solve(int device, const double* l1, int64_t N1, const double* l2, int64_t N2, double n_eff, double tol, int32_t maxit,
                           int32_t on_device, double* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_BRIDGE_H */
