/*
 * logreg_hip_ppc.h -- posterior predictive checks from replicated outcomes, on the device: replicate the outcomes under every draw and
 * ask whether the observed data look like the replicates (Gelman, Meng & Stern 1996; bayesplot's pp_check / ppc_stat_grouped).  WAIC,
 * LOO and the evidence rank models against each other; this says whether one model is adequate, and for which group of rows it is not.
 *
 * Inputs.
 *     check rows x_i (i < r)   the model's own resident rows and labels (X_new = NULL, as lr_predict_create), or host X_new [r,p] with
 *                              optional labels y_new
 *     group labels g_i         in [0, G), optional (NULL: every row in group 0, G = 1); G <= LR_PPC_MAX_GROUPS = 32
 *     seed                     64 bits, the accumulator's own
 * Draws beta_s are indexed by s = the number of draws handed to the accumulator before this one ([iters, C, p] flattened time-major).
 *
 * Per (draw, row) pair, in the model's dtype with the arithmetic of lr_predict's pairs:
 *     eta = x_i . beta_s       sequential fma over the coordinates
 *     e   = exp(-|eta|)        one exponential and one log1p(e) serve everything below
 *     pi  = sigma(eta)         1 / (1 + e) or e / (1 + e), never 1 - sigma
 *     l_1 = log sigma(eta)  = min(eta, 0) - log1p(e)
 *     l_0 = log sigma(-eta) = min(-eta, 0) - log1p(e)
 *
 * Replicate.  y_rep(s,i) = [u < pi], false for a NaN operand.  u = ((w >> 8) + 0.5) 2^-24, the 24-bit uniform of logreg_hip.h formed in
 * the model's dtype (a float32 model rounds the 25-bit sum to even: its u differs from the float64 one by 2^-25, and is 1 for the
 * last of the 2^24 values), w = word (s & 3) of the Philox4x32-10 block with key = seed and counter = (q lo, q hi, i, LR_PPC_TAG), q = s >> 2: one
 * block serves a row for four consecutive draws.  LR_PPC_TAG = 0x04000000 is free beside the normal blocks (small integers), 0x08000000
 * (bridge), 0x10000000 (PG), 0x20000000 / 0x40000000 (NUTS) and 0x80000000 (the accept uniform).  y_rep depends on (seed, s, i, pi)
 * alone: not on how the draws are cut into calls or pieces, nor on the lane or the kind of pointer.
 *
 * Per draw.
 *     T_g(s)   = sum over the rows of group g of y_rep(s,i)          an integer
 *     D_obs(s) = -2 sum_i l_{y_i}                                    NaN without labels, and everything derived from it
 *     D_rep(s) = -2 sum_i l_{y_rep(s,i)}
 * The row sums are float64 in a fixed order: a fixed tree inside a tile of 256 rows, then the tiles in ascending order.
 *
 * Accumulated.
 *     hist[g][k]   uint64, k = 0 .. n_g   the draws with T_g = k  (n_g = the rows of group g; the groups' runs follow each other:
 *                                         group g starts at sum_{h < g} (n_h + 1), r + G cells in all)
 *     row_ones[i]  uint64                 sum_s y_rep(s,i)
 *     counts[0]    uint64  dev_ge         the draws with D_rep >= D_obs
 *     counts[1]    uint64  n_nonfinite
 *     moments[0..3]  mean and M2 (sum of squared deviations) of D_obs, then of D_rep, over the finite draws; batches are merged by
 *                  the pairwise rule of Chan, Golub & LeVeque as lr_predict's
 *     n_draws      every draw handed over, the non-finite ones included
 * A draw with a non-finite coordinate adds to n_nonfinite alone.  It still consumes its index s: the stream positions of later draws
 * do not move.
 *
 * Invariance.  The integer tables (hist, row_ones, counts) are exact: byte-identical however the draws are cut into calls or pieces,
 * in both builds, for host and device pointers.  The moments are byte-identical for the same sequence of calls and equal within
 * float64 rounding otherwise.  No float atomics anywhere; the integer ones commute.
 *
 * A header of its own, as logreg_hip_predict.h: the entry points are bound from their own table (logreg_amd/_lib.py PPC_SYMBOLS).
 * Status codes, lr_last_error and the pointer conventions are those of logreg_hip.h.  An accumulator reads its model's rows: it may be
 * DESTROYED after the model, but not used; like the model handle it is not thread-safe.
 */
#ifndef LOGREG_HIP_PPC_H
#define LOGREG_HIP_PPC_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_PPC_MAX_GROUPS 32
#define LR_PPC_TAG 0x04000000u
#define LR_PPC_MOMENTS 4

typedef struct lr_ppc lr_ppc;

/*
 * X_new   [r,p] host doubles (rounded to the model's dtype), or NULL = the model's own design and labels: then r must be the model's n
 *         and y_new must be NULL.
 * y_new   [r] host doubles in {0,1}, or NULL = no labels (D_obs and what derives from it are NaN, the observed T_g are -1).
 * groups  [r] host int32 in [0, G), or NULL = one group (G must then be 1).
 * Errors (with a reason, ahead of any device access): NULL model / out, r <= 0 or beyond 2^31 - 1, r != n with X_new = NULL, y_new
 * without X_new, non-finite X_new, labels outside {0,1}, a group label outside [0, G), G outside 1 .. LR_PPC_MAX_GROUPS.
 */
LR_API int lr_ppc_create(lr_model* m, const double* X_new, const double* y_new, int64_t r, const int32_t* groups, int32_t G, uint64_t seed,
                         lr_ppc** out);

/*
 * Fold S draws in, as lr_predict_accumulate: draws [S,p] in the model's dtype, host memory (on_device = 0: the call returns when the
 * work is done) or device memory (on_device = 1: enqueued on `stream`).  Errors: NULL arguments, S <= 0.  Running out of memory leaves
 * the accumulator as it was.  The workspace of per-tile partials does not grow with S: a piece is worked off in sub-batches of draws
 * whose size depends on (r, G) alone.
 */
LR_API int lr_ppc_accumulate(lr_ppc* pc, const void* draws, int64_t S, int32_t on_device, void* stream);

/*
 * hist [r + G] and row_ones [r] uint64, counts [2] uint64, moments [LR_PPC_MOMENTS] doubles (NaN while no finite draw was seen; rows 0
 * and 1 NaN without labels), t_obs [G] (the observed T_g; -1 without labels) and n_g [G] int64, n_draws: all host memory, each may be
 * NULL.  Synchronises with the stream of the last accumulate call.
 */
LR_API int lr_ppc_result(lr_ppc* pc, uint64_t* hist, uint64_t* row_ones, uint64_t* counts, double* moments, int64_t* t_obs, int64_t* n_g,
                         int64_t* n_draws);

/*
 * The per-draw quantities of S draws taken as s = first_index, first_index + 1, ...; nothing is accumulated.  Host outputs:
 * counts_out [S,G] int32 (T_g), dev_out [S,2] float64 (D_obs, D_rep) and, unless NULL, yrep_out [S, ceil(r / 32)] uint32 (bit i & 31 of
 * word i >> 5 is y_rep(s,i); the bits past r are 0).  A draw with a non-finite coordinate gives zero counts and bits and NaN twice.
 * Errors: NULL accumulator / draws / counts_out / dev_out, S <= 0, first_index < 0.
 */
LR_API int lr_ppc_terms(lr_ppc* pc, const void* draws, int64_t S, int64_t first_index, int32_t on_device, void* stream, int32_t* counts_out,
                        double* dev_out, uint32_t* yrep_out);

/* Forget every draw (the next one is s = 0 again).  The rows, labels, groups and the seed stay. */
LR_API int lr_ppc_reset(lr_ppc* pc);

LR_API void lr_ppc_destroy(lr_ppc* pc);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_PPC_H */
