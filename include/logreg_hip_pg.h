/*
 * logreg_hip_pg.h -- the Polya-Gamma Gibbs sampler of liblogreg_hip.so: the exact data-augmentation sampler of Polson, Scott & Windle
 * (2013) for Bayesian logistic regression with a Gaussian prior, many chains fused into one kernel launch, on the models of logreg_hip.h.
 * It has no tuning constant, no accept step and no warm-up.
 *
 * The reference's tuning-free script is R/fit-rjags.R (a JAGS Gibbs sampler on the same model); lr_run_pg is the library's counterpart.
 *
 * A header of its own: logreg_hip.h's symbol set is pinned by the test double of the whole ABI; the entry points below are bound from
 * their own table (logreg_amd/_lib.py PG_SYMBOLS).  Every convention of logreg_hip.h holds (status codes, lr_last_error, lr_run_opts,
 * host / device pointers, the counter-based random stream), with these differences:
 *   - opts->precision is IGNORED: the draw runs in the model's dtype and the linear algebra in float64, whatever it says;
 *   - there is no lp_state and no accept count: every sweep moves the chain (or leaves it in place and counts it, see `skipped`);
 *   - a run is planned as ONE part, rows in LDS on 16 lanes per chain (LR_MODE_LDS, group 16): p > 32, n >= 65 536, and rows + the
 *     omega staging beyond the LDS return LR_ERR_UNSUPPORTED with the reason.
 *
 * ---- One sweep of chain c at global iteration t.  xs_i = (2 y_i - 1) x_i are the signed rows, pscale_j the prior sd (prior mean 0).
 *   1. psi_i = xs_i . beta for every row (the model's dtype, coordinates in ascending order, fused multiply-adds).
 *   2. omega_i ~ PG(1, |psi_i|) for every row: "The draw" below, in the model's dtype.
 *   3. A = sum_i omega_i xs_i xs_i^T + diag(1 / pscale^2) in float64, rows in ascending order:
 *          A_jk <- fma(omega_i, xs_ij * xs_ik, A_jk), then A_jj += 1 / pscale_j^2.
 *      b = 1/2 sum_i xs_i = X^T (y - 1/2) does not depend on the state: computed once per model on the host, in float64.
 *   4. d_j = 1 / sqrt(A_jj), R_jk = A_jk (d_j d_k) (unit diagonal up to rounding), R = L L^T by Cholesky (column by column, every pivot
 *      must be finite and > 0), L y = D b, L^T x = y + z, beta <- D x.  That is beta = A^-1 b + (A^-1/2 factor) z ~ N(A^-1 b, A^-1).
 *      z: the p standard normals of normal blocks 0 .. ceil(p/4) - 1, as lr_run_hmc draws its momentum.
 *      All of 3 and 4 is float64 for both model dtypes; the new state is rounded to the model's dtype when stored.
 * A chain with a non-finite psi_i, or with a pivot that is not finite and > 0, stays where it is for that iteration: `skipped` gains 1
 * and the iteration adds nothing to the other two counters.
 *
 * ---- The draw: Devroye's exact sampler of J*(1, z), z = |psi| / 2, truncation point t = 0.64; omega = X / 4.
 * Constants: K = pi^2 / 8 + z^2 / 2;  Phi(x) = erfc(-x / sqrt 2) / 2;
 *   r = 0                                                                                       if z >= 10
 *   r = 1 / (1 + (4 / pi) K (exp(K t - z) Phi((t z - 1) / sqrt t) + exp(K t + z) Phi(-(t z + 1) / sqrt t)))    otherwise
 * r is the weight of the right (exponential-tail) proposal.  The second line is the textbook weight; for z < 10 its largest exponent
 * is K t + z < 43, so nothing overflows in float32, and the smallest Phi is erfc(6.6) / 2 ~ 1e-20, a normal float32.  For z >= 10 the
 * textbook value is below 1 / (1 + (4 / pi) 51 exp(22.8) / 2) < 2^-38, and a 24-bit uniform is never below 2^-25: the comparison
 * U < r is false for every word, so r = 0 draws exactly the same omega as the textbook weight and no exponent is ever formed.
 * a_n(x) = pi (n + 1/2) (2 / (pi x))^(3/2) exp(-2 (n + 1/2)^2 / x)  for x <= t,   pi (n + 1/2) exp(-(n + 1/2)^2 pi^2 x / 2)  for x > t.
 *
 * Random stream: the row's own sub-stream.  Philox4x32-10, key = seed, counter = (chain, iter_lo, iter_hi, block) with
 *   block = LR_PG_TAG | (b << 16) | i,   i the row (< 65 536), b = 0, 1, ... (< 4096) the row's 4-word blocks in the order consumed.
 * The words of blocks 0, 1, ... form one sequence w_0, w_1, ... (w_k = word k % 4 of block k / 4) read by a cursor that only moves
 * forward; u(w) = ((w >> 8) + 1/2) 2^-24 is the 24-bit uniform of logreg_hip.h.  The range is disjoint from the normal blocks (< 2^16),
 * LR's uniform tag 0x80000000 and the two NUTS tags (0x40000000 | d, 0x20000000 | k with d, k < 2^16 -- bit 28 is clear in all of them).
 *
 *   round (at most LR_PG_MAX_ROUNDS = 10):
 *     U = u(next word).  The proposal is the right one if U < r.
 *     right:  E = -ln u(next word);  X = t + E / K.
 *     left:   trials of exactly three words (a, b, c) each, at most LR_PG_MAX_TRIALS = 160:
 *        z < 1 / t (exponential pair):  E1 = -ln u(a), E2 = -ln u(b);  X = t / (1 + t E1)^2;
 *                                       the trial succeeds if E1^2 <= 2 E2 / t  and  u(c) <= exp(-z^2 X / 2).
 *        otherwise (Michael-Schucany-Haas, mu = 1 / z):  N = sqrt(-2 ln u(a)) cos(2 pi u(b)),  w = mu N^2 / 2,  s = 1 + w + sqrt(w (w + 2)),
 *                                       X = mu / s;  if u(c) > mu / (mu + X): X = mu s;   the trial succeeds if X <= t.
 *                                       (mu / s is the root mu + mu^2 N^2 / 2 - mu sqrt(4 mu N^2 + mu^2 N^4) / 2 without its cancellation)
 *        At the bound the last trial's X, or t if that is larger, is taken as if the trial had succeeded.
 *     V = u(next word);  S = a_0(X);  Y = V S;  then for n = 1, 2, ..., LR_PG_MAX_TERMS = 8:
 *        n odd:  S -= a_n(X);  if Y <= S the draw ends with omega = X / 4.
 *        n even: S += a_n(X);  if Y > S the round is rejected and the next one starts.
 *        At the bound the draw ends with omega = X / 4.
 *   After LR_PG_MAX_ROUNDS rejected rounds the draw ends with omega = X / 4 of the last round.
 * Every comparison is written so that a NaN operand reads as "false"; every loop ends at its bound whatever the values.
 *
 * The bounds, each from its loop's per-pass acceptance lower bound, each far below one draw in 10^24:
 *   series    a term n is reached only if Y lies between two partial sums a_n(X) apart; Y is uniform on [0, a_0(X)], so the chance is
 *             a_n / a_0 <= (2 n + 1) exp(-2 n (n + 1) / t) (x <= t) or (2 n + 1) exp(-n (n + 1) pi^2 t / 2) (x > t): at n = 8 below e^-220.
 *   rounds    Devroye's proposal accepts with probability >= 1 / 1.0009 for every z, so ten rejections have probability < (9e-4)^10 < 1e-30.
 *   pair      P(E1^2 <= 2 E2 / t) = int exp(-x - t x^2 / 2) dx = 0.723 and exp(-z^2 X / 2) >= exp(-z^2 t / 2) > exp(-1 / (2 t)) = 0.458 for
 *             z < 1 / t: a trial succeeds with probability >= 0.331, 160 fail with probability < 0.669^160 < 2e-28.
 *   MSH       P(X <= t) for the inverse Gaussian (mu <= t, lambda = 1) is smallest at mu = t: 1/2 + e^(2 / t) Phi(-2 / sqrt t) = 0.641;
 *             160 failures have probability < 0.36^160 < 1e-70.
 * A draw consumes at most 10 (2 + 3 * 160) words = 1205 blocks < 4096.  omega is finite and positive for every finite psi with
 * |psi| <= 1e15 in float32 and 1e150 in float64 (beyond, 1 / z^2-sized quantities leave the normal range).
 *
 * omega_i depends on (seed, chain, iteration, row, psi_i) alone: not on the lane that drew it, the chunking of a run or the shard a
 * chain runs in.  A is summed in row order, so neither do the states.
 */
#ifndef LOGREG_HIP_PG_H
#define LOGREG_HIP_PG_H

#include "logreg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lr_plan_run / lr_plan_run_info: the kernel family of lr_run_pg */
#define LR_KIND_PG 6
#define LR_PG_TAG 0x10000000u
#define LR_PG_MAX_ROUNDS 10
#define LR_PG_MAX_TRIALS 160
#define LR_PG_MAX_TERMS 8
#define LR_PG_MAX_ROWS 65536 /* n < LR_PG_MAX_ROWS: the row index takes 16 bits of the block number */

/* Per-chain counters of lr_run_pg: every call ADDS to what the array holds (zero it once before a run). */
typedef struct lr_pg_counters {
    uint64_t proposals;    /* rounds of the draw, over all rows and iterations (theory: <= 1.0009 per row and iteration) */
    uint64_t series_terms; /* terms a_n, n >= 1, evaluated by the alternating-series test */
    uint32_t skipped;      /* iterations that left the chain in place (a non-finite psi, or a pivot that is not finite and > 0) */
    uint32_t reserved;
} lr_pg_counters;

/*
 * Every call advances all chains by iters * thin sweeps.
 *   state     [C,p]  in/out
 *   out       [iters,C,p] or NULL    row i = states after (i+1)*thin sweeps
 *   counters  [C] or NULL            added to
 * opts->stats (streaming statistics) as for the other samplers; opts->precision is ignored.
 */
LR_API int lr_run_pg(lr_model* m, void* state, const lr_run_opts* opts, void* out, lr_pg_counters* counters);

/*
 * The omega of step 2 for the iteration at opts->iter_offset, without moving the state: the test surface of the draw.
 *   state      [C,p]  read only
 *   omega_out  [C,n]  in the model's dtype; NaN where psi_i is not finite
 * opts->iters and opts->thin are not read.
 */
LR_API int lr_pg_omega(lr_model* m, const void* state, const lr_run_opts* opts, void* omega_out);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_PG_H */
