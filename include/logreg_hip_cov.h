/*
 * logreg_hip_cov.h -- the joint structure of the kept draws of liblogreg_hip.so, without taking them off the device: a streaming
 * accumulator of the second cross-moment of blocks [k, C, p] of draws in time order (any sampler's).  It keeps, per chain, the sum of
 * every coordinate and, pooled over chains and time, the p x p matrix of cross products: what cor(out) of the reference's
 * Python/analyse.R:17 needs -- and, because the chains stay apart in the sums, the within- and between-chain covariance matrices and the
 * multivariate R-hat of Brooks & Gelman (1998) too.  Covariance, correlation, W, B, R-hat and a diagonal metric are formed on the host
 * (logreg_amd/covariance.py) from the four tables below.
 *
 * Definitions.  Every draw x is first converted to double.  center_j and scale_j > 0 are fixed at creation.
 *
 * u.       u_j = (x_j - center_j) * scale_j: one subtraction, then one multiplication (nothing here may contract to an fma).  With
 *          center near the posterior mean and scale = 1 / sd, |u| is about 1: a posterior far from 0 costs no digits in
 *          M - s s^T / N.  Coordinates p .. P - 1 of the kernel's padded width P carry u = 0 and add exactly nothing.
 *
 * Chain sums (persistent state, C p doubles).  S[c][j] += u_j, per series (chain, coordinate), in time order.
 *
 * Moment.  With P = LR_COV_WIDTH(p), the pairs (absolute time index t = 0, 1, ... since creation or reset; chain c) are cut into cells
 *              cell(t, c) = (c / G, t mod R)           R = LR_COV_RESIDUES(P): 25 for P <= 32, 7 for P = 64, 1 for P = 128
 *                                                      G = LR_COV_CHUNK(P) * 2^e, e >= 0 the smallest with ceil(C / G) <= LR_COV_GROUPS(P)
 *          -- a function of (C, p) alone: never of k or of how the draws were cut into calls.  Inside a cell entry (i, j), i <= j, takes
 *          one M_ij = fma(u_i, u_j, M_ij) per draw, the draws in (t, c) order.  The cells are persistent state.  lr_cov_result adds the
 *          cells in cell order (g R + r): runs of 64 consecutive cells are summed one after the other, then the runs' sums one after the
 *          other.  No float atomics.  moment is returned full and symmetric.
 *
 * chain_outer.  Q[i][j] = sum_c S[c][i] S[c][j], i <= j: runs of LR_COV_OUTER_RUN = 128 consecutive chains, Q = fma(S_ci, S_cj, Q) per
 *          chain in chain order, then the runs' sums one after the other; returned full and symmetric.  sum[j] = sum_c S[c][j]: the same
 *          runs, one addition per chain, then the runs in order.
 *
 * Same bytes.  The same draws give the same bytes of all four tables however they were cut into calls, from host or device memory,
 *          after a reset, and in every build of the library.
 *
 * Non-finite draws.  A NaN or +-inf draw of coordinate j makes S[c][j] of its chain, sum[j] and rows and columns j of moment and
 *          chain_outer non-finite (0 * inf and 0 * NaN are NaN too) -- never a finite wrong number -- and touches no other entry.
 *
 * With n = 0 draws all four tables are NaN.
 *
 * A header of its own, as logreg_hip_marginals.h: logreg_hip.h's symbol set is pinned; the entry points below are bound from their own
 * table (logreg_amd/_lib.py COV_SYMBOLS).  Status codes, lr_last_error and the pointer and stream conventions are those of
 * logreg_hip.h / logreg_hip_marginals.h.  An accumulator is not thread-safe.
 */
#ifndef LOGREG_HIP_COV_H
#define LOGREG_HIP_COV_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_COV_MAX_P 128
/* the kernel's padded width, the time residues of the cell partition, the chains staged together, the most chain groups */
#define LR_COV_WIDTH(p) ((p) <= 4 ? 4 : (p) <= 8 ? 8 : (p) <= 16 ? 16 : (p) <= 32 ? 32 : (p) <= 64 ? 64 : 128)
#define LR_COV_RESIDUES(P) ((P) <= 32 ? 25 : (P) == 64 ? 7 : 1)
#define LR_COV_CHUNK(P) ((P) <= 32 ? 128 / (P) : (P) == 64 ? 8 : 32)
#define LR_COV_GROUPS(P) ((P) == 4 ? 4096 : (P) == 8 ? 2048 : (P) == 16 ? 1024 : 512)
#define LR_COV_CELL_RUN 64
#define LR_COV_OUTER_RUN 128

typedef struct lr_cov lr_cov;

/*
 * C chains x p coordinates (1..LR_COV_MAX_P) of draws of `dtype` (LR_F32 / LR_F64) on `device`; center [p], scale [p] host doubles,
 * finite, scale > 0.  Errors (with a reason): NULL out / center / scale, C or p out of range, a bad dtype, a bad center or scale, out of
 * memory.
 */
LR_API int lr_cov_create(int device, int32_t dtype, int64_t C, int32_t p, const double* center, const double* scale, lr_cov** out);

/*
 * Fold k more time steps in.  block [k, C, p] in the accumulator's dtype, rows in time order, host memory (on_device = 0: staged, and
 * the call returns when the work is done) or device memory (on_device = 1: enqueued on `stream`; the buffer may be reused or freed
 * once the stream has passed this call).  All calls on one accumulator must use one stream, or be ordered by the caller.
 * Errors: NULL arguments, k <= 0, out of memory -- which leaves the accumulator as it was (the staging buffer is sized before
 * anything is folded in).
 */
LR_API int lr_cov_accumulate(lr_cov* h, const void* block, int64_t k, int32_t on_device, void* stream);

/*
 * moment [p, p], chain_outer [p, p], sum [p], chain_sums [C, p]: host doubles, each may be NULL; n_draws (may be NULL) receives n, the
 * time steps folded in so far.  Synchronises with the stream of the last accumulate call; the state is not changed (more draws may
 * follow).
 */
LR_API int lr_cov_result(lr_cov* h, double* moment, double* chain_outer, double* sum, double* chain_sums, int64_t* n_draws);

/* Forget every draw (n = 0); center and scale stay. */
LR_API int lr_cov_reset(lr_cov* h);

LR_API void lr_cov_destroy(lr_cov* h);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_COV_H */
