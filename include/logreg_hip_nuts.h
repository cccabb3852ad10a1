/*
 * logreg_hip_nuts.h -- the No-U-Turn sampler of liblogreg_hip.so: many chains of multinomial NUTS (Hoffman & Gelman 2014; the
 * iterative, checkpointed form of Phan, Pradhan & Jankowiak 2019) fused into one kernel launch, on the models of logreg_hip.h.
 *
 * The reference's library scripts run NUTS with a diagonal metric and no warm-up:
 *     Python/fit-blackjax-nuts.py:101   blackjax.nuts(lpost, 1e-3, pre), pre = [10,1,1,1,1,1,5,1], 10 000 iterations
 *     Python/fit-numpyro.py:36-46       numpyro NUTS on the same model
 * lr_run_nuts replaces their sampler loop.  BlackJAX's `inverse_mass_matrix = pre` is this call's dmm = 1 / pre.  (The warm-up that
 * finds eps and dmm -- fit-numpyro.py:44 `num_warmup=1000` -- is logreg_hip_adapt.h.)
 *
 * A header of its own: logreg_hip.h's symbol set is pinned by the test double of the whole ABI; the entry points below are bound
 * from their own table (logreg_amd/_lib.py NUTS_SYMBOLS).  Every convention of logreg_hip.h holds (status codes, lr_last_error,
 * lr_run_opts, host / device pointers, the counter-based random stream), with these differences:
 *   - opts->precision is read as LR_PREC_FULL: every leapfrog step of a NUTS trajectory is a leaf whose energy enters the
 *     multinomial weights and the U-turn and divergence decisions, so no evaluation may be computed more cheaply;
 *   - there is no lp_state: the log-posterior at the current state is recomputed at the start of every call;
 *   - a run is always planned as ONE part (lr_plan_info.split = 0): the trees of a wave run in lockstep, and a second variant
 *     for the remainder of a chain count would not shorten the longest tree;
 *   - the fused kernel keeps the data rows in LDS (LR_MODE_LDS, 16 lanes per chain): under LR_MODE_AUTO shapes with no such variant
 *     -- p > 32, rows beyond the LDS -- return LR_ERR_UNSUPPORTED with the reason, which names the mode that takes them:
 *   - opts->mode = LR_MODE_STEPWISE runs lr_run_nuts on the stepwise engine for exactly those shapes -- p > 32 (up to 128), or rows and
 *     checkpoints at LR_NUTS_MAX_DEPTH beyond the LDS; a shape the fused kernel takes keeps refusing this mode, as it always did:
 *     per leapfrog step one evaluation over all row slices and one update launch that does the tree bookkeeping (lr_tall_nuts.h).  All
 *     chains of the call build their trees in lockstep, so every building chain is at the same leaf of the same doubling.  The plan
 *     is the stepwise plan of the other samplers (lr_plan_info: mode stepwise, group = row slices, rows = slice length, one part;
 *     opts->group pins the slice count and with it the order of the sums).  The same random stream: the same Markov chain as the
 *     fused kernel up to the order of the sums.  What differs for the caller:
 *       . the call is NOT a pure enqueue.  At the end of every doubling but the last possible one the host reads, on opts->stream, how
 *         many chains are still building, and ends the iteration when none is: up to max_depth - 1 waits per iteration, each a
 *         synchronisation of that stream.  All work stays on that stream; the loop is bounded by 2^max_depth - 1 steps whatever is
 *         read, and the results do not depend on when the host looks (a finished chain applies nothing).  It cannot be captured
 *         into a graph;
 *       . workspace: behind the stepwise engine's own, (15 + 2 max_depth) x C x P elements of the model's type (P = p padded to 4, 8,
 *         16, 32, 64 or 128) + 112 bytes per chain (224 at P = 128), kept per (model, stream) like the engine's; LR_ERR_NOMEM with the byte count;
 *       . at most 65535 x 64 chains per call, as for every run on the stepwise engine;
 *       . the diagonal metric only: lr_run_nuts_dense and the warm-up (logreg_hip_adapt.h) refuse LR_MODE_STEPWISE and p > 32.
 *     LR_MODE_AUTO never chooses this path.
 *
 * Random stream (DESIGN.md "NUTS"): Philox4x32-10, key = seed, counter = (chain, iter_lo, iter_hi, block):
 *   momentum      normal blocks 0 .. ceil(p/4) - 1, as lr_run_hmc draws it
 *   doubling d    block 0x40000000 | d  (LR_NUTS_TAG_TREE): word x bit 31 = direction (1: forward), word y = merge uniform
 *   leaf k        word k % 4 of block 0x20000000 | (k / 4)  (LR_NUTS_TAG_LEAF): the progressive-sampling uniform of the k-th
 *                 leapfrog step of the iteration, counted from 0 across the whole tree
 */
#ifndef LOGREG_HIP_NUTS_H
#define LOGREG_HIP_NUTS_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lr_plan_run / lr_plan_run_info: the kernel family of lr_run_nuts */
#define LR_KIND_NUTS 4
#define LR_NUTS_TAG_TREE 0x40000000u
#define LR_NUTS_TAG_LEAF 0x20000000u
#define LR_NUTS_MAX_DEPTH 10

/* Per-chain counters of lr_run_nuts: every call ADDS to what the array holds (zero it once before a run). */
typedef struct lr_nuts_counters {
    uint64_t n_leapfrog;      /* leapfrog steps (= gradient evaluations) */
    uint64_t depth_sum;       /* sum over iterations of the tree depth (doublings made) */
    double accept_stat_sum;   /* sum over iterations of the mean over the tree's leaves of min(1, exp(H0 - H)) */
    uint32_t divergent;       /* iterations that ended in a divergence (H - H0 > 1000 or a non-finite H) */
    uint32_t max_depth_hits;  /* iterations that ended because the tree reached max_depth (neither turning nor divergent) */
} lr_nuts_counters;

/*
 * NUTS with diagonal metric: p ~ N(0, dmm), H = -lpost(q) + 1/2 sum p^2 / dmm, q += eps * p / dmm (the reference HMC's convention,
 * Python/fit-np-hmc.py:65-87).  Every call advances all chains by iters * thin iterations.
 *   state     [C,p]  in/out
 *   eps       leapfrog step, finite and > 0
 *   max_depth 1 .. LR_NUTS_MAX_DEPTH: at most 2^max_depth - 1 leapfrog steps per iteration
 *   dmm       [p]    host doubles, finite and > 0
 *   out       [iters,C,p] or NULL    row i = states after (i+1)*thin iterations
 *   counters  [C] or NULL            added to
 *   depth_out [iters,C] int8 or NULL the tree depth of the iteration that produced row i, negated when it diverged
 * opts->stats (streaming statistics) as for the other samplers.
 */
LR_API int lr_run_nuts(lr_model* m, void* state, double eps, int32_t max_depth, const double* dmm, const lr_run_opts* opts, void* out,
                       lr_nuts_counters* counters, int8_t* depth_out);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_NUTS_H */
