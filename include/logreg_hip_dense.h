/*
 * logreg_hip_dense.h -- the No-U-Turn sampler of liblogreg_hip.so (logreg_hip_nuts.h) under a DENSE metric: Stan's metric=dense_e,
 * NumPyro's dense_mass=True, BlackJAX's matrix `inverse_mass_matrix` (the reference's Python/fit-blackjax-nuts.py:101 and
 * Python/fit-numpyro.py:36-46 pass a diagonal one; a matrix in that place is this call's inv_metric).
 *
 * Definition.  The caller passes the INVERSE metric Sigma [p][p], symmetric positive definite, approximately the posterior covariance
 * (BlackJAX's inverse_mass_matrix).  lr_run_nuts' dmm corresponds to Sigma = diag(1 / dmm).
 *     momentum   p ~ N(0, Sigma^-1)
 *     energy     H = -lpost(q) + 1/2 p^T Sigma p
 *     position   q += eps Sigma p
 *     U-turn     generalised, rho' = rho - (p_a + p_b) / 2:  turning when p_a . (Sigma rho') <= 0 or p_b . (Sigma rho') <= 0
 * The random stream, the tree, the checkpoints, progressive sampling, the divergence rule, the counters and depth_out are those of
 * lr_run_nuts, unchanged (logreg_hip_nuts.h; DESIGN.md "NUTS").
 *
 * Factorisation (lr_dense_factor): pure host code in float64, every operation written out, nothing contracted, sums in ascending
 * index order; only the LOWER triangle of inv_metric (row-major, element [i * p + j], j <= i) is read.
 *     s_j   = sqrt(Sigma_jj)
 *     R_ij  = Sigma_ij / (s_i * s_j) for j < i, R_ji = R_ij, R_ii = 1                         (the correlation matrix)
 *     L     = Cholesky-Banachiewicz of R, row by row:  t = R_ij - sum_{k<j} L_ik L_jk (k ascending, one subtraction per term);
 *             L_ii = sqrt(t),  L_ij = t / L_jj (j < i)
 *     A     = L^-T by back substitution, column c = 0 .. p-1, i = c .. 0:  t = (i == c ? 1 : 0) - sum_{i<k<=c} L_ki A_kc (k ascending);
 *             A_ic = t / L_ii;  A_ic = 0 for i > c
 * The momentum of an iteration is p = (A z) / s with z the normals exactly as lr_run_nuts draws them; the velocity is
 * v = s o (R (s o p)).  The device receives (T) s, (T)(1 / s), (T) R and (T) A.  The correlation-scaled form keeps the momentum's
 * covariance and the kinetic energy's matrix consistent after rounding to float32: their mismatch is of the order cond(R) * 2^-24
 * whatever the scales of Sigma are.
 * Refused (LR_ERR_INVALID, with the reason, before any device access): an entry of the lower triangle that is not finite, a diagonal
 * entry that is not > 0, a pivot t of a diagonal element that is not > 0 (Sigma is not positive definite).
 *
 * A diagonal Sigma gives the dynamics of lr_run_nuts with dmm = 1 / diag(Sigma): the same decisions, states equal within rounding (not
 * bytes: p . (c p) and (p . p) c round differently).
 *
 * A header of its own, as logreg_hip_nuts.h: logreg_hip.h's symbol set is pinned; the entry points below are bound from their own table
 * (logreg_amd/_lib.py DENSE_SYMBOLS).  Every convention of logreg_hip_nuts.h holds.
 */
#ifndef LOGREG_HIP_DENSE_H
#define LOGREG_HIP_DENSE_H

#include "logreg_hip.h"
#include "logreg_hip_nuts.h"
#include "logreg_hip_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The factorisation above.  p in 1 .. 32; inv_metric [p][p] host doubles; s [p], R [p][p], A [p][p] host doubles, each may be NULL.
 * No device is touched.
 */
LR_API int lr_dense_factor(int32_t p, const double* inv_metric, double* s, double* R, double* A);

/*
 * lr_run_nuts under the dense metric: every argument but inv_metric [p][p] (host doubles, always) as lr_run_nuts', with the same
 * conventions -- host or device pointers by opts->on_device, opts->stats, results independent of how a run is cut into calls or its
 * chains into shards, opts->precision read as LR_PREC_FULL.  The kernel keeps R and A in LDS beside the rows and the U-turn
 * checkpoints (2 P P values more, P the padded width): a shape beyond the LDS is refused with LR_ERR_UNSUPPORTED and the reason.
 * The model keeps the device image of the last factor per stream: a call with the inv_metric of the call before it on the same stream
 * enqueues without a host synchronisation; a call with another one first waits for that stream.
 */
LR_API int lr_run_nuts_dense(lr_model* m, void* state, double eps, int32_t max_depth, const double* inv_metric, const lr_run_opts* opts,
                             void* out, lr_nuts_counters* counters, int8_t* depth_out);

/*
 * Warm-up under a dense metric: logreg_hip_adapt.h with the full inverse metric in place of the diagonal one.
 *
 * Step size.  Dual averaging exactly as logreg_hip_adapt.h defines it (the statistic, the order of its sums, the constants, the restart
 * rule, the Philox base LR_ADAPT_ITER_BASE + t), every iteration run by the dense kernel at the current Sigma: iteration t IS
 * lr_run_nuts_dense(iters = 1, thin = 1, iter_offset = LR_ADAPT_ITER_BASE + t) with the trace's eps_t and the Sigma of the last window
 * that ended before t (inv_metric before the first).
 *
 * Metric.  The windows are lr_adapt_schedule's.  In a window every iteration's states x [C][p] (float64) enter one pooled
 * (n, mean [p], M [p][p]) over chains and time, M_jl the co-moment of coordinates j and l.  With P = LR_ADAPT_WIDTH(p), Q = 256 / P:
 *     workgroup b = chains 256 b .. min(256 b + 255, C - 1), n_b of them, i = 0 .. n_b - 1:
 *         mean_b as in logreg_hip_adapt.h;  for every pair l <= j:  e[q] = fma(d_ij, d_il, e[q]) from 0.0 over i = q, q + Q, ...
 *         (ascending), d_ij = x_ij - mean_b_j;  tree: for s = Q/2, .. 1: e[q] += e[q + s], q < s;  M_b_jl = e[0]
 *     merge (Chan et al.) a <- b:  n = n_a + n_b, d = mean_b - mean_a,
 *         M_jl = fma(d_j * d_l, n_a * n_b / n, M_a_jl + M_b_jl),   mean_j = fma(d_j, n_b / n, mean_a_j)
 *     the workgroups in the order b = 0, 1, ..., then the iteration's triple INTO the window's (an empty window takes it as it is), the
 *     iterations in order.  The diagonal M_jj is logreg_hip_adapt.h's M2_j, operation for operation.
 * At a window's last iteration, after the step-size update, on the host in float64 (the one host synchronisation of the warm-up; at
 * most LR_ADAPT_MAX_WINDOWS of them, five at W = 1000; between window ends everything is enqueued back to back):
 *     S = M / (n - 1);   Sigma = (n / (n + 5)) * S + 1e-3 * (5 / (n + 5)) * I;   lr_dense_factor(Sigma)
 * A Sigma that lr_dense_factor refuses keeps the previous metric and is counted in lr_adapt_info.metric_skipped (windows, not
 * coordinates).  The window's triple is emptied and dual averaging restarts from eps_{t+1}, as in logreg_hip_adapt.h.
 *
 * opts->adapt_metric = 0: the step size alone under the fixed inv_metric -- a metric that comes from elsewhere (a Laplace
 * approximation, the covariance of a pilot run) needs its step re-tuned.  opts->dmm0 must be NULL; inv_metric NULL is the unit metric.
 *
 * The handle is an lr_adapt and the contracts of lr_adapt_create / _run / _result / _trace / _destroy hold: everything a call allocates
 * is allocated before anything is enqueued, a failed handle stays failed, and the trace, the metrics, the final eps and every state
 * depend only on (seed, chain_offset, start states, options) -- not on how W was cut into calls, on the build or on the pointer kind.
 */
LR_API int lr_dense_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* opts, const double* inv_metric, lr_adapt** out);
LR_API int lr_dense_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* opts, void* out,
                              lr_nuts_counters* counters, int8_t* depth_out, double* astat_out);
/* eps, inv_metric [p][p] (host doubles: the current Sigma), info: each may be NULL; as lr_adapt_result */
LR_API int lr_dense_adapt_result(lr_adapt* h, double* eps, double* inv_metric, lr_adapt_info* info);
/* trace [W][LR_ADAPT_TRACE_COLS], metric [n_windows][p][p] (Sigma after each window; rows of windows not yet run are 0): host doubles */
LR_API int lr_dense_adapt_trace(lr_adapt* h, double* trace, double* metric);
LR_API void lr_dense_adapt_destroy(lr_adapt* h);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_DENSE_H */
