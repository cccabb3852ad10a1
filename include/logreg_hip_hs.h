/*
 * logreg_hip_hs.h -- the horseshoe Polya-Gamma Gibbs sampler of liblogreg_hip.so: Bayesian logistic regression under the (regularised)
 * horseshoe prior of Carvalho, Polson & Scott (2010), sampled by the Polya-Gamma augmentation of logreg_hip_pg.h with the scales as further
 * Gibbs blocks in the auxiliary-variable form of Makalic & Schmidt (2016).  Many chains fused into one kernel launch; no tuning constant,
 * no accept step, no warm-up.
 *
 * A header of its own (bound from logreg_amd/_lib.py HS_SYMBOLS).  Every convention of logreg_hip_pg.h holds: opts->precision is ignored,
 * there is no lp_state, a run is planned exactly as lr_run_pg plans it (LR_KIND_PG: the same LDS footprint, the same refusals; the
 * sampler is not a kind of lr_plan_run).
 *
 * ---- The model.  S is the set of shrunk coordinates (prior->shrink[j] != 0), m = |S|, tau0 = prior->global_scale > 0.
 *
 *   pi(beta, lambda, tau | y)  ~  L(beta)  prod_j N(beta_j; 0, pscale_j^2)  prod_{j in S} N(beta_j; 0, tau^2 lambda_j^2) C+(lambda_j; 0, 1)  C+(tau; 0, tau0)
 *
 * The model's own Gaussian N(0, pscale_j^2) stays on EVERY coordinate.  On a shrunk coordinate it is the slab of the regularised
 * horseshoe (Piironen & Vehtari 2017) in the "fictitious data" form of Nishimura & Suchard (2022): a factor of the target beside the
 * horseshoe's normal, not a reparametrisation of its scale, so the conditionals of lambda and tau stay inverse-gamma.  An unshrunk
 * coordinate keeps exactly the prior of logreg_hip_pg.h.  The half-Cauchys are written with auxiliaries:
 *      lambda_j^2 | nu_j ~ IG(1/2, 1 / nu_j),   nu_j ~ IG(1/2, 1);        tau^2 | xi ~ IG(1/2, 1 / xi),   xi ~ IG(1/2, 1 / tau0^2).
 *
 * ---- The hyper-state of a chain: 2 p + 2 doubles,  lambda^2 [p], nu [p], tau^2, xi  (entries of unshrunk coordinates are carried, never
 * read by the model).  Every entry a caller passes must be finite and in [LR_HS_MIN, LR_HS_MAX]; from host memory anything else is
 * refused, in device memory (opts->on_device) it is read as step 7 would have left it (clamped; a NaN as 1).
 *
 * ---- One sweep of chain c at global iteration t, from (beta, hyper-state).  Steps 1-4 are those of logreg_hip_pg.h.
 *   1. psi and omega: the operations and the row sub-streams of lr_run_pg, so omega is the omega lr_run_pg draws at the same
 *      (seed, chain, iteration, row, psi).
 *   2. A as in logreg_hip_pg.h, except that the diagonal gains  ivar_j + s_j * ((1 / tau^2) * (1 / lambda_j^2)),  ivar_j = 1 / pscale_j^2,
 *      s_j = 1.0 for j in S and 0.0 otherwise: a multiplier, not a branch.  With S empty every sum is ivar_j + 0.0 and the states are
 *      lr_run_pg's byte for byte.
 *   3. Scaling, factorisation, the two solves and z: logreg_hip_pg.h step 4.
 *   4. The skip rule of logreg_hip_pg.h.  A skipped sweep leaves the hyper-state in place as well, and counts no clamp.
 *   With the NEW beta as stored (rounded to the model's dtype), in float64, u53 and the blocks as under "Random stream":
 *   5. for j in S:   lambda_j^2 <- (1 / nu_j + beta_j^2 * (0.5 * (1 / tau^2))) / E1_j          (tau^2: the value the sweep started with)
 *                    nu_j       <- (1 + 1 / lambda_j^2) / E2_j                                  (lambda_j^2: the new, clamped value)
 *   6. Q = sum_{j in S} beta_j^2 * (1 / lambda_j^2), new lambda.  Order of the sum: the partial sums q_r = sum over j = r, r + 16 (j in S,
 *      ascending) for r = 0 .. 15, then the 16 partial sums by the butterfly of group_sum<16>:
 *      a_i = q_i + q_{15 - i};  b_i = a_i + a_{(i & 8) | (7 - (i & 7))};  c_i = b_i + b_{i ^ 2};  Q = c_0 + c_1.
 *                    tau^2 <- (1 / xi + 0.5 * Q) / G,     G = sum_{k < floor((m + 1) / 2)} E_k  (+ z^2 / 2 if m + 1 is odd)
 *      The E_k are summed by the same butterfly, with e_k = E_k for k < floor((m + 1) / 2) and 0 otherwise (m <= 32, so k < 16), and
 *      z^2 / 2 is added last.  G ~ Gamma((m + 1) / 2, 1).
 *                    xi    <- (1 / tau0^2 + 1 / tau^2) / E3                                      (tau^2: the new, clamped value)
 *   7. Every new value is clamped to [LR_HS_MIN, LR_HS_MAX] = [1e-100, 1e100] as it is formed, and each clamp adds 1 to the chain's
 *      `clamped`.  A NaN leaves the old value in place and counts as a clamp.  The clamp keeps 1 / (tau^2 lambda_j^2) finite, so one
 *      extreme draw cannot pin a chain on the skip rule forever.
 *
 * ---- Random stream of the hyper-step.  Philox4x32-10, key = seed, counter = (chain, iter_lo, iter_hi, LR_HS_TAG | b), words (w0 .. w3):
 *      b = j < 32              (w0, w1) -> E1_j,  (w2, w3) -> E2_j
 *      b = LR_HS_BLOCK_GLOBAL  (w0, w1) -> E3,    (w2, w3) -> z = sqrt(-2 ln u32(w2)) cos(2 pi u32(w3)),   u32(w) = (w + 1/2) 2^-32
 *      b = LR_HS_BLOCK_GAMMA + k / 2, k < 16:   (w0, w1) -> E_k for even k,  (w2, w3) -> E_k for odd k
 * E = -ln u53(wa, wb) with  u53 = (((wa >> 5) 2^26 + (wb >> 6)) + 1/2) 2^-53  in float64: a 53-bit uniform (the sum in parentheses is an
 * exact integer; adding 1/2 rounds to nearest even from 2^52 up).  A 24-bit uniform would put the inverse-gamma tail -- the horseshoe's
 * tail -- on a grid.  LR_HS_TAG is disjoint from every other tag of the library (csrc/lr_device.h lists them).
 *
 * The new hyper-state depends on (seed, chain, iteration, the new beta, the old hyper-state, the prior) alone: not on the lane that drew
 * it, the chunking of a run or the shard a chain runs in.
 *
 * ---- The empty set.  lr_run_hs and lr_hs_hyper ACCEPT m = 0 (every shrink[j] zero): the states are then lr_run_pg's byte for byte
 * (the test of that identity is the reason), and tau^2, xi move under their priors (G = z^2 / 2).  The Python face refuses an empty
 * mask: that model is pgKernel's.
 */
#ifndef LOGREG_HIP_HS_H
#define LOGREG_HIP_HS_H

#include "logreg_hip_pg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LR_HS_TAG 0x02000000u
#define LR_HS_BLOCK_GLOBAL 32
#define LR_HS_BLOCK_GAMMA 33
#define LR_HS_MIN 1e-100
#define LR_HS_MAX 1e100

typedef struct lr_hs_prior {
    const uint8_t* shrink; /* [p] host memory: nonzero = the coordinate is shrunk */
    double global_scale;   /* tau0: finite and > 0 */
} lr_hs_prior;

/* Per-chain counters: the layout of lr_pg_counters, its reserved word in use.  Every call ADDS to what the array holds. */
typedef struct lr_hs_counters {
    uint64_t proposals;    /* as lr_pg_counters */
    uint64_t series_terms; /* as lr_pg_counters */
    uint32_t skipped;      /* as lr_pg_counters */
    uint32_t clamped;      /* step 7 */
} lr_hs_counters;

/*
 * Every call advances all chains by iters * thin sweeps.
 *   state      [C,p]  in/out, the model's dtype
 *   hyper      [C,2p+2] float64, in/out
 *   out        [iters,C,p] or NULL      row i = states after (i+1)*thin sweeps
 *   scale_out  [iters,C,p+1] float64 or NULL   with row i of out: lambda_j^2 for j < p (1.0 where unshrunk), tau^2 at index p
 *   counters   [C] or NULL              added to
 * prior (and prior->shrink) are host memory whatever opts->on_device says.  opts->stats as for lr_run_pg.
 * Refused before any device access: a NULL argument that is not optional, global_scale not finite and > 0, and (host memory) a hyper
 * entry that is not finite and in [LR_HS_MIN, LR_HS_MAX]; then everything lr_run_pg refuses.
 */
LR_API int lr_run_hs(lr_model* m, const lr_hs_prior* prior, void* state, double* hyper, const lr_run_opts* opts, void* out, double* scale_out,
                     lr_hs_counters* counters);

/*
 * Steps 5-7 alone for the iteration at opts->iter_offset, moving nothing: the test surface of the hyper-step.
 *   state      [C,p]  read only (the "new beta" of step 5)
 *   hyper_in   [C,2p+2] read only
 *   hyper_out  [C,2p+2]
 *   counters   [C] or NULL: `clamped` is added to, nothing else
 * opts->iters and opts->thin are not read.
 */
LR_API int lr_hs_hyper(lr_model* m, const lr_hs_prior* prior, const void* state, const double* hyper_in, const lr_run_opts* opts, double* hyper_out,
                       lr_hs_counters* counters);

#ifdef __cplusplus
}
#endif
#endif /* LOGREG_HIP_HS_H */
