/*
 * logreg_hip_adapt_tall.h -- the NUTS warm-up of logreg_hip_adapt.h on the stepwise engine: for the models lr_run_nuts samples with
 * mode = LR_MODE_STEPWISE (logreg_hip_nuts.h) -- 32 < p <= 128, or a narrow model whose rows and U-turn checkpoints at LR_NUTS_MAX_DEPTH do
 * not fit the LDS -- which lr_adapt_create refuses.
 *
 * Definitions.  Everything logreg_hip_adapt.h states holds here word for word: the schedule, the acceptance statistic, abar_t through
 * sum256, dual averaging, the pooled (n, mean_j, M2_j) with Chan merges in workgroup order, the window-end metric, the restarts; float64
 * everywhere, nothing contracted, no float atomics.  One extension: the lane map of the metric's partial sums goes on beyond 32 lanes,
 *     P = LR_ADAPT_TALL_WIDTH(p) = LR_ADAPT_WIDTH(p) for p <= 32, 64 for 32 < p <= 64, 128 for 64 < p <= 128;     Q = 256 / P
 * so a wide model sums the chains of a workgroup in Q = 4 or Q = 2 lane-strided sequences, joined by the same tree over Q
 * (s = Q/2, .. 1: s[q] += s[q + s]).
 *
 * Contract.  Iteration t of a warm-up IS lr_run_nuts(iters = 1, thin = 1, iter_offset = LR_ADAPT_ITER_BASE + t, mode = LR_MODE_STEPWISE,
 * the same group) with the float64 (eps_t, dmm_t) of the trace, bit for bit.  The trace, the metric, the final eps and every state depend
 * only on (seed, chain_offset, start states, options, C, and the slice plan: opts->group and plan_chains) -- not on how the W iterations
 * were cut into lr_tall_adapt_run calls, not on the build of the library, not on whether pointers are host or device.
 *
 * A handle of lr_tall_adapt_create is an lr_adapt: lr_adapt_result, lr_adapt_trace and lr_adapt_destroy serve it unchanged.  lr_adapt_run
 * refuses it, and lr_tall_adapt_run refuses a handle of lr_adapt_create.  The entry points are bound from their own table
 * (logreg_amd/_lib.py ADAPT_TALL_SYMBOLS).
 */
#ifndef LOGREG_HIP_ADAPT_TALL_H
#define LOGREG_HIP_ADAPT_TALL_H

#include "logreg_hip_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_ADAPT_TALL_WIDTH(p) ((p) <= 32 ? LR_ADAPT_WIDTH(p) : (p) <= 64 ? 64 : 128)

/*
 * lr_adapt_create's arguments and argument checks.  The model must be one lr_run_nuts takes with mode = LR_MODE_STEPWISE; a shape the
 * fused kernel takes is refused with LR_ERR_UNSUPPORTED, and the text names lr_adapt_create as its path.
 */
LR_API int lr_tall_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* opts, lr_adapt** out);

/*
 * lr_adapt_run's arguments and semantics, with these differences.  opts->mode must be LR_MODE_STEPWISE (anything else: LR_ERR_UNSUPPORTED,
 * before any device access); opts->group asks a slice count, as for lr_run_nuts.  The chains stay in the engine's workspace across the
 * iterations of one call: the states are loaded and evaluated once at its start and stored once at its end.  The call is SYNCHRONOUS in the
 * way lr_run_nuts is on this engine: at the end of every doubling of every iteration the host reads, on opts->stream, how many chains are
 * still building; an iteration is bounded by 2^max_depth - 1 leaves whatever is read.  So the call is NOT graph-capturable, with device
 * pointers as with host pointers.  Everything the call allocates (the engine's workspace, the staging of host arrays) is allocated before
 * anything is enqueued: LR_ERR_NOMEM leaves the handle as it was.  A launch that fails part-way (LR_ERR_HIP) marks the handle failed, as
 * lr_adapt_run does.
 */
LR_API int lr_tall_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* opts, void* out,
                             lr_nuts_counters* counters, int8_t* depth_out, double* astat_out);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_ADAPT_TALL_H */
