/*
 * logreg_hip_adapt.h -- the warm-up of the No-U-Turn sampler of liblogreg_hip.so (logreg_hip_nuts.h): Stan-style windowed adaptation
 * of ONE step size and ONE diagonal metric shared by all C chains of a run, pooled over the chains on the device.  The reference's
 * Python/fit-numpyro.py:44 runs MCMC(kernel, num_warmup=1000, ...); this is that warm-up for lr_run_nuts.
 *
 * Definitions.  A warm-up runs W iterations of all C chains.  Iteration t = 0 .. W-1 is one NUTS iteration of every chain with the
 * current (eps, dmm), at Philox iteration index LR_ADAPT_ITER_BASE + t (= 2^62 + t): a sampling run that counts from 0 never reuses a
 * warm-up counter.  The (seed, chain, iteration) contract of the random stream holds as in logreg_hip_nuts.h: iteration t of a
 * warm-up IS lr_run_nuts(iters = 1, thin = 1, iter_offset = LR_ADAPT_ITER_BASE + t) with the float64 (eps_t, dmm_t) of the trace.
 *
 * Schedule (lr_adapt_schedule; Stan's windowed schedule; a pure function of W, init_buffer = 75, term_buffer = 50, base_window = 25):
 *     W < 20: step size only, no metric window.
 *     if init + base + term > W:  init = floor(0.15 W), term = floor(0.10 W), base = W - init - term.
 *     start = init, size = base; while start < W - term:
 *         end = start + size; if end + 2 size > W - term: end = W - term      (the window after it would not end by W - term)
 *         the window is [start, end); start = end, size = 2 size.
 *     W = 1000 -> ends 100, 150, 250, 450, 950.   W = 150 -> 100.   W = 60 -> init 9, one window ending at 54.
 *     Iterations before init and from W - term on adapt the step size only.  adapt_metric = 0: no windows.
 *
 * Acceptance statistic.  a[c] = the iteration's mean over the tree's leaves of min(1, exp(H0 - H)) of chain c -- what
 * lr_nuts_counters.accept_stat_sum accumulates; 0 for a divergent first leaf (a chain whose state is not finite contributes 0).
 *     sum256(v): 256 slots (0.0 for a chain beyond C); for s = 128, 64, .. 1: v[i] += v[i + s], i < s; the result is v[0].
 *     abar_t = (sum256 of chains 0..255 + sum256 of chains 256..511 + ..., added in this order) / C.        All float64.
 *
 * Step size (Hoffman & Gelman 2014, dual averaging), float64, one operation per operator as written, nothing contracted; m = iterations
 * since the last restart counted from 1:
 *     Hbar        = (1 - 1 / (m + t0)) * Hbar + (delta - abar_t) / (m + t0)
 *     log_eps     = mu - sqrt(m) / gamma * Hbar
 *     eta         = pow(m, -kappa)
 *     log_eps_bar = eta * log_eps + (1 - eta) * log_eps_bar
 *     eps_{t+1}   = exp(log_eps)
 * Start and restart: mu = log(10 eps), Hbar = 0, log_eps_bar = 0, m = 0, with eps = eps0 at the start and eps = eps_{t+1} after the
 * metric update of iteration t.  After iteration W - 1 the reported step is exp(log_eps_bar).  Defaults: gamma 0.05, t0 10, kappa 0.75,
 * delta 0.8.  (exp, log and pow are the device library's: within a few ulp of any other; the trace records what was used.)
 *
 * Metric.  In a window every iteration's states x [C][p] (converted to float64 whatever the model's dtype) enter a pooled running
 * (n, mean_j, M2_j) per coordinate j, over chains and time.  With P = LR_ADAPT_WIDTH(p) and Q = 256 / P, per iteration:
 *     workgroup b = chains 256 b .. min(256 b + 255, C - 1), n_b of them, numbered i = 0 .. n_b - 1:
 *         s[q]   = 0.0 + x_i + x_{i+Q} + ...  for i = q, q + Q, ... (ascending);    tree: for s = Q/2, .. 1: s[q] += s[q + s], q < s
 *         mean_b = s[0] / n_b
 *         e[q]   = fma(d_i, d_i, e[q]) from e[q] = 0.0 over the same i, d_i = x_i - mean_b;   the same tree;   M2_b = e[0]
 *     merge (n_a, mean_a, M2_a) <- (n_b, mean_b, M2_b) (Chan et al.):  n = n_a + n_b, d = mean_b - mean_a,
 *         mean = fma(d, n_b / n, mean_a),   M2 = fma(d * d, n_a * n_b / n, M2_a + M2_b)
 *     the workgroups are merged in the order b = 0, 1, ...; the iteration's triple is then merged INTO the window's (a = window,
 *     b = iteration; an empty window takes the iteration's triple as it is), the iterations in order.
 * At a window's last iteration, after the step-size update:  var_j = M2_j / (n - 1);
 *     inv_metric_j = (n / (n + 5)) * var_j + 1e-3 * (5 / (n + 5));    dmm_j = 1 / inv_metric_j
 * (this library's convention is p ~ N(0, dmm): BlackJAX's `pre`, NumPyro's inverse mass matrix, is inv_metric = 1 / dmm).  A
 * coordinate whose var_j is not finite or not > 0 keeps its dmm_j and is counted in lr_adapt_info.metric_skipped.  The window's
 * triple is emptied and dual averaging restarts.  No float atomics anywhere.
 *
 * The kernel's tuning of iteration t + 1 is formed from the float64 values exactly as lr_run_nuts forms it on the host:
 * (T) eps, (T) sqrt(dmm_j), (T)(eps / dmm_j), (T)(1 / dmm_j).
 *
 * Contract.  The trace, the metric, the final eps and every state depend only on (seed, chain_offset, start states, options) -- not on
 * how the W iterations were cut into lr_adapt_run calls, not on the build of the library, not on whether pointers are host or device.
 * They DO depend on C: the adaptation pools over the chains of the handle.  A shard of a larger run adapts by itself.
 *
 * A header of its own, as logreg_hip_cov.h: logreg_hip.h's symbol set is pinned; the entry points below are bound from their own table
 * (logreg_amd/_lib.py ADAPT_SYMBOLS).  Status codes, lr_last_error and the pointer and stream conventions are those of logreg_hip.h.  A
 * handle is not thread-safe; all calls on one handle must use one stream, or be ordered by the caller.
 */
#ifndef LOGREG_HIP_ADAPT_H
#define LOGREG_HIP_ADAPT_H

#include "logreg_hip.h"
#include "logreg_hip_nuts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_ADAPT_ITER_BASE (INT64_C(1) << 62)
#define LR_ADAPT_MAX_WINDOWS 32
#define LR_ADAPT_TRACE_COLS 5 /* eps used, abar_t, log_eps_bar after the step (before a restart), window index or -1, the window's n or 0 */
#define LR_ADAPT_WIDTH(p) ((p) <= 4 ? 4 : (p) <= 8 ? 8 : (p) <= 16 ? 16 : 32)

typedef struct lr_adapt lr_adapt;

typedef struct lr_adapt_opts {
    int32_t W;             /* warm-up iterations, >= 1 */
    int32_t adapt_metric;  /* 0: step size only (dmm0 stays) */
    double delta;          /* target mean acceptance statistic in (0, 1); 0 = 0.8 */
    double eps0;           /* first step, finite and > 0; 0 = 1 */
    const double* dmm0;    /* [p] host doubles, finite and > 0, or NULL for the unit metric */
    double gamma, t0, kappa; /* dual averaging; 0 = 0.05, 10, 0.75 */
    int32_t init_buffer, term_buffer, base_window; /* 0 = 75, 50, 25; negative values are refused */
    int32_t reserved;
} lr_adapt_opts;

typedef struct lr_adapt_info {
    int64_t iterations;     /* warm-up iterations done */
    int64_t metric_skipped; /* coordinates whose window variance was not finite or not > 0, summed over the windows done */
    int32_t windows;        /* metric windows done */
    int32_t n_windows;      /* metric windows of the schedule */
} lr_adapt_info;

/*
 * The schedule alone: pure host code, no device.  ends [LR_ADAPT_MAX_WINDOWS] receives the exclusive window ends, *n_windows their
 * count, *init_out (may be NULL) the first iteration of the first window.  Buffers: 0 = default.  Errors: NULL ends / n_windows, W < 1,
 * a negative buffer.
 */
LR_API int lr_adapt_schedule(int32_t W, int32_t init_buffer, int32_t term_buffer, int32_t base_window, int32_t* ends, int32_t* n_windows,
                             int32_t* init_out);

/*
 * A warm-up of C chains of model m (which must outlive the handle).  Argument errors are refused, with the reason, before any device
 * access, p > 32 among them (LR_ERR_UNSUPPORTED, as lr_run_nuts); lr_run_nuts' other refusals (a forced mode or lane count, rows and
 * checkpoints beyond the LDS at the call's max_depth) come from lr_adapt_run, which plans the kernel.  Out of memory: LR_ERR_NOMEM.
 */
LR_API int lr_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* opts, lr_adapt** out);

/*
 * Advance the warm-up by iters <= remaining iterations (0: nothing).  state [C,p] in/out; out [iters,C,p], counters [C] (added to),
 * depth_out [iters,C], astat_out [iters,C] float64 (the acceptance statistics a[c]) are optional (NULL).  Host or device pointers by
 * opts->on_device, as lr_run_nuts; device pointers: three launches per iteration are enqueued on opts->stream, with no host
 * synchronisation.  Read from opts: n_chains (must be C), chain_offset, seed, group, mode, on_device, stream.  opts->iters, thin and
 * iter_offset are IGNORED; opts->stats must be NULL (refused).  Everything the call allocates is allocated before anything is enqueued:
 * LR_ERR_NOMEM (like every refused argument) leaves the handle as it was.  A kernel launch that fails part-way (LR_ERR_HIP) does not: the
 * iterations enqueued before it stand, the handle is marked failed and every later lr_adapt_run on it returns LR_ERR_HIP; lr_adapt_result
 * and lr_adapt_trace still read what was computed.
 */
LR_API int lr_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* opts, void* out,
                        lr_nuts_counters* counters, int8_t* depth_out, double* astat_out);

/*
 * eps, dmm [p] (host doubles), info: each may be NULL.  After W iterations eps is exp(log_eps_bar); before, the step the next
 * iteration will use.  Synchronises with the stream of the last lr_adapt_run.
 */
LR_API int lr_adapt_result(lr_adapt* h, double* eps, double* dmm, lr_adapt_info* info);

/*
 * trace [W][LR_ADAPT_TRACE_COLS], metric [n_windows][2][p] (row 0: var, row 1: dmm after the window): host doubles, each may be NULL.
 * Rows of iterations / windows not yet run are 0.
 */
LR_API int lr_adapt_trace(lr_adapt* h, double* trace, double* metric);

LR_API void lr_adapt_destroy(lr_adapt* h);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_ADAPT_H */
