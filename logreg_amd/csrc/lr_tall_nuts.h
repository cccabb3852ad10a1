// lr_tall_nuts.h -- NUTS on the stepwise engine (tall n, and wide models 32 < p <= 128): the tree bookkeeping of nuts_run (lr_nuts.h)
// between two evaluations, as one update launch per leaf.  The evaluation itself is the engine's: launch_tall_partial(value, grad) at
// q1 (lr_tall.h, lr_wide_*.h), summed here in slice order (tall_reduced_grad / tall_reduced_value).
//
// Layout as k_tall_update: lane = coordinate, P lanes per chain, 256-lane blocks; every sum over the coordinates (kinetic energies,
// U-turn dot products) is chain_sum<P>, identical in the P lanes of a chain, so every decision is the same in all of them.
//
// Lockstep over the WHOLE launch.  All chains of a call start an iteration together and a building chain takes one leaf per launch;
// a subtree ends early only through a divergence or a U-turn, and both end the tree.  So every chain that is still building is at the
// same doubling d and leaf i, and the host passes them (lr_nuts_sched.h): the checkpoint indices, the leaf-uniform word and the end of
// a doubling are uniform over the grid, and every branch around a chain_sum<P> (which synchronises the block for P > 64) is taken by
// all threads or by none.  A chain whose tree is finished applies nothing: every store is behind its `done` flag, and its q1 stays
// where it is, so the evaluations the launch still makes for it change nothing.  Leaf k of DESIGN.md is step s for every chain: the
// random stream is k_nuts's, and the Markov chain is k_nuts's up to the order of the sums.
//
// Phases (NutsTallPhase):
//   NPH_BEGIN  start of iteration `iter` (flag = 1: after the evaluation at x, also zeroing the call's counters; otherwise reached
//              through NPH_END from the carried x, g, lp): momentum, H0, doubling 0's direction and merge uniform, the moving end, the
//              first half kick and drift -> q1
//   NPH_LEAF   (s, d, i; flag = 1: count the chains still building into tally[d]) everything nuts_run does after `evaluate` for leaf s,
//              then everything before `evaluate` for leaf s + 1
//   NPH_END    the iteration's counters, x, g, lp for the next one, the kept row (out_row >= 0); flag = 1: NPH_BEGIN of iter + 1
//   NPH_STORE  the state back, the counters added to the caller's
//   NPH_CARRY  (TUNED only) NPH_BEGIN of `iter` from the carried x, g, lp that NPH_END with flag = 0 left, as a launch of its own
//
// TUNED (k_tall_nuts_update_tuned; the warm-up: include/logreg_hip_adapt_tall.h): step, a, b, c come from a NutsTune block in device memory, which k_adapt_update
// (lr_adapt.h) rewrites between NPH_END of one iteration and NPH_CARRY of the next, and NPH_END writes astat [C], what acc_sum gains.
#pragma once

#include "lr_nuts.h"
#include "lr_nuts_sched.h"
#include "lr_tall.h"

namespace lr {

enum NutsTallPhase { NPH_BEGIN = 0, NPH_LEAF = 1, NPH_END = 2, NPH_STORE = 3, NPH_CARRY = 4 };
// the tree's vectors [C][P] in the workspace; the checkpoints (momentum, partial momentum sum) of index k follow at NTV_COUNT + 2 k
enum NutsTallVec { NTV_LQ, NTV_LP, NTV_LG, NTV_RQ, NTV_RP, NTV_RG, NTV_CP, NTV_RHO, NTV_RHOS, NTV_PFIRST, NTV_PINNER, NTV_PX, NTV_PG, NTV_SX, NTV_SG, NTV_COUNT };
static_assert(NTV_COUNT == kNutsTallVecs, "lr_nuts_sched.h sizes the workspace");
enum NutsTallFlag { NTF_DONE = 1, NTF_DIV = 2, NTF_TURNED = 4, NTF_FWD = 8 };

struct NutsTallChain {  // per-chain scalars of the tree and the call's counters
    double lp, plp, slp, H0, W, Ws, sumacc, umerge, acc_sum;
    uint64_t n_leap, depth_sum;
    uint32_t n_div, n_hit;
    int32_t nleaf, depth, flags;
};
static_assert(sizeof(NutsTallChain) == kNutsTallChainBytes, "lr_nuts_sched.h sizes the workspace");

template <typename T> struct NutsTallArgs {
    T* v;                // [NTV_COUNT + 2 max_depth][C][P]
    NutsTallChain* ch;   // [C][waves per chain]
    uint32_t* tally;     // [kNutsTallSlots]: chains still building after the last leaf of doubling d
    NutsCounters* counters;  // the caller's [C], added to by NPH_STORE, or null
    int8_t* depth_out;       // the caller's [iters][C] or null
    int max_depth;
};

// ... and those of the TUNED instantiation; NutsTallArgs keeps its layout
template <typename T, int P> struct NutsTallTunedArgs : NutsTallArgs<T> {
    const NutsTune<T, P>* tune;
    double* astat;  // [C]: the acceptance statistic of the iteration NPH_END closes
};
template <typename T, int P, bool TUNED> using NutsTallArgsOf = std::conditional_t<TUNED, NutsTallTunedArgs<T, P>, NutsTallArgs<T>>;

// One body (lr_tall_nuts_update.inc) under two kernels: the plain one keeps its name and signature; the TUNED one takes the derived arguments.
// Inside the body `if constexpr (TUNED)` discards what the other kernel's arguments do not have.
template <typename T, int P>
__global__ void __launch_bounds__(256) k_tall_nuts_update(TallArgs<T, P> a, NutsTallArgs<T> n, int phase, int64_t iter, int s, int d, int i, int64_t out_row, int flag) {
    constexpr bool TUNED = false;
#include "lr_tall_nuts_update.inc"
}
template <typename T, int P>
__global__ void __launch_bounds__(256) k_tall_nuts_update_tuned(TallArgs<T, P> a, NutsTallTunedArgs<T, P> n, int phase, int64_t iter, int s, int d, int i, int64_t out_row,
                                                                int flag) {
    constexpr bool TUNED = true;
#include "lr_tall_nuts_update.inc"
}

// the launch of InstTable::launch_tall_nuts (TUNED: launch_tall_nuts_tuned, nuts_args a NutsTallTunedArgs) for one (dtype, padded p); d, i outside the tree of max_depth: -1, nothing launched
template <typename T, int P, bool TUNED = false>
int launch_tall_nuts_t(hipStream_t st, const void* tall_args, const void* nuts_args, int phase, int64_t iter, int s, int d, int i, int64_t out_row, int flag) {
    const auto& a = *static_cast<const TallArgs<T, P>*>(tall_args);
    const auto& n = *static_cast<const NutsTallArgsOf<T, P, TUNED>*>(nuts_args);
    if (n.max_depth < 1 || n.max_depth > kNutsMaxDepth || phase < NPH_BEGIN || phase > (TUNED ? NPH_CARRY : NPH_STORE)) return -1;
    if (phase == NPH_LEAF && (d < 0 || d >= n.max_depth || i < 0 || i >= (1 << d) || s != (1 << d) - 1 + i)) return -1;
    const dim3 grid((unsigned)((a.C * P + 255) / 256)), block(256);
    if constexpr (TUNED) hipLaunchKernelGGL((k_tall_nuts_update_tuned<T, P>), grid, block, 0, st, a, n, phase, iter, s, d, i, out_row, flag);
    else hipLaunchKernelGGL((k_tall_nuts_update<T, P>), grid, block, 0, st, a, n, phase, iter, s, d, i, out_row, flag);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace lr
