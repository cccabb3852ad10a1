// lr_nuts.h -- the fused many-chain No-U-Turn sampler: one launch runs `iters x thin` iterations of multinomial NUTS for every chain
// (include/logreg_hip_nuts.h; the algorithm, its random stream and the lockstep scheme: DESIGN.md "NUTS").
//
// Layout as k_chain_dist (lr_kernels.h): one chain per 16-lane DPP row, lane r owns coordinates r + 16 k (for P < 16 lanes r >= P
// hold zeros); rows staged in LDS.  Sums over the coordinates (kinetic energies, U-turn dot products) are group_sum<16> over the row,
// bit-identical in its 16 lanes, so every decision is the same in all lanes of a chain.
//
// Lockstep.  A wave holds 4 chains whose trees differ in size.  The iteration is ONE loop over leapfrog steps: at step s every lane
// takes a step from its chain's moving end and evaluates the log-posterior there, whether or not its chain is still building; a chain
// whose tree is finished applies nothing (every update is a select on its `done` flag, as k_chain's `acc ? xp : x`).  No branch that
// can differ between the chains of a wave surrounds an evaluation, a DPP move or a draw; the loop leaves when no chain of the wave is
// building (a ballot), and after 2^max_depth - 1 steps whatever the values -- a NaN, an infinity or a stuck chain cannot hang it.
// Because every building chain takes one step per pass, the leaf counter k of DESIGN.md is the step index s for every chain.
//
// The U-turn checkpoints (momentum and partial momentum sum per bit count of the leaf index) are indexed at run time, so they live in
// LDS after the rows: 2 x max_depth x P / 16 values per lane -- in registers they would go to scratch, which the build refuses.
#pragma once

#include <type_traits>

#include "lr_kernels.h"

namespace lr {

// stream tags of NUTS (lr_device.h "Philox4x32-10"; include/logreg_hip_nuts.h)
constexpr uint32_t TAG_NUTS_TREE = 0x40000000u;  // | d: doubling d -- word x bit 31 = direction, word y = merge uniform
constexpr uint32_t TAG_NUTS_LEAF = 0x20000000u;  // | k / 4: word k % 4 = progressive-sampling uniform of leaf k
constexpr int kNutsMaxDepth = 10;

struct NutsCounters {  // lr_nuts_counters
    uint64_t n_leapfrog, depth_sum;
    double accept_stat_sum;
    uint32_t divergent, max_depth_hits;
};

template <typename T, int P> struct NutsArgs {
    T* state;                // [C][p] in/out
    T* out;                  // [iters][C][p] or null
    NutsCounters* counters;  // [C] added to, or null
    int8_t* depth_out;       // [iters][C] or null
    int64_t C, chain_offset, iters, thin, iter_offset;
    uint64_t seed;
    int p, max_depth;
    T step;                  // eps
    T a[P], b[P], c[P];      // sqrt(dmm), eps / dmm, 1 / dmm (zero in padded coordinates)
    StatsArgs stats;
};

// The tuning of NutsArgs (step, a, b, c) as a block in device memory, and the arguments of the TUNED instantiation of k_nuts, which reads
// it from there: the warm-up (include/logreg_hip_adapt.h, lr_adapt.h) rewrites the block between the launches of consecutive iterations
// and reads `astat` [C], the acceptance statistic of the launch's last iteration.  NutsArgs keeps its layout.
template <typename T, int P> struct NutsTune {
    T step;
    T a[P], b[P], c[P];
};
template <typename T, int P> struct NutsTunedArgs : NutsArgs<T, P> {
    const NutsTune<T, P>* tune;
    double* astat;
};
template <typename T, int P, bool TUNED> using NutsArgsOf = std::conditional_t<TUNED, NutsTunedArgs<T, P>, NutsArgs<T, P>>;

// dynamic LDS of k_nuts beyond the rows: the checkpoints of a 256-lane workgroup
template <typename T, int P> constexpr size_t nuts_ckpt_bytes(int max_depth) { return (size_t)2 * max_depth * ((P + 15) / 16) * 256 * sizeof(T); }

// P < 16: all[j] = coordinate j from lane j of the row (row_share)
template <typename T, int P, int S = 0> __device__ __forceinline__ void nuts_gather_small(T own, T (&all)[P]) {
    if constexpr (S < P) {
        all[S] = dpp_mov<0x150 + S>(own);
        nuts_gather_small<T, P, S + 1>(own, all);
    }
}

__device__ __forceinline__ uint32_t lane_word(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_ds_bpermute(lane * 4, (int)v); }

__device__ __forceinline__ double nuts_lae(double a, double b) {  // log(exp(a) + exp(b)), both finite
    const double mx = a > b ? a : b, d = a > b ? b - a : a - b;
    return mx + log1p(exp(d));
}

// The metric as a policy of the tree loop (nuts_run): what the loop asks of it is the momentum of a draw, the position update of a
// leapfrog step, the kinetic energy and the generalised U-turn criterion.  NutsDiagMetric is the diagonal metric of
// include/logreg_hip_nuts.h; NutsDenseMetric (lr_nuts_dense.h) the full matrix of include/logreg_hip_dense.h.  Every sum over the
// coordinates is group_sum<16> in both.
template <typename T, int P, bool TUNED> struct NutsDiagMetric {
    static constexpr int NK = (P + 15) / 16;
    using Args = NutsArgsOf<T, P, TUNED>;
    T ca[NK], cb[NK], cc[NK];
    // (lds: the workgroup's LDS behind the checkpoints -- the diagonal metric keeps nothing there)
    __device__ __forceinline__ void load(const Args& a, int r, T* lds) {
        (void)lds;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = r + 16 * k, js = j < P ? j : 0;
            if constexpr (TUNED) {
                ca[k] = j < P ? a.tune->a[js] : T(0);
                cb[k] = j < P ? a.tune->b[js] : T(0);
                cc[k] = j < P ? a.tune->c[js] : T(0);
            } else {
                ca[k] = j < P ? a.a[js] : T(0);
                cb[k] = j < P ? a.b[js] : T(0);
                cc[k] = j < P ? a.c[js] : T(0);
            }
        }
    }
    // p = sqrt(dmm) z
    __device__ __forceinline__ void momentum(const T (&z)[NK], T (&pm)[NK]) const {
#pragma unroll
        for (int k = 0; k < NK; ++k) pm[k] = z[k] * ca[k];
    }
    // q += +-eps p / dmm (eps is folded into cb)
    __device__ __forceinline__ void drift(bool fwd, T step, const T (&pm)[NK], T (&q)[NK]) const {
        (void)step;
#pragma unroll
        for (int k = 0; k < NK; ++k) q[k] = fma_t(fwd ? cb[k] : -cb[k], pm[k], q[k]);
    }
    // generalised U-turn criterion: rho' = rho - (pa + pb) / 2; (pa / dmm) . rho' <= 0 or (pb / dmm) . rho' <= 0
    __device__ __forceinline__ bool turning(const T (&pa)[NK], const T (&pb)[NK], const T (&rh)[NK]) const {
        T sa = T(0), sb = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const T rr = fma_t(T(-0.5), pa[k] + pb[k], rh[k]);
            sa = fma_t(cc[k] * pa[k], rr, sa);
            sb = fma_t(cc[k] * pb[k], rr, sb);
        }
        sa = group_sum<16>(sa);
        sb = group_sum<16>(sb);
        return sa <= T(0) || sb <= T(0);
    }
    __device__ __forceinline__ double kinetic2(const T (&pm)[NK]) const {  // sum p^2 / dmm
        T s = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) s = fma_t(pm[k] * pm[k], cc[k], s);
        return (double)group_sum<16>(s);
    }
};

// the whole kernel but its name: k_nuts and k_nuts_dense (lr_nuts_dense.h) are this body under their metric
template <typename T, int P, int MODE, int R, bool TUNED, typename Metric>
__device__ __forceinline__ void nuts_run(const ModelArgs<T, P>& m, const typename Metric::Args& a) {
    static_assert(MODE == MODE_LDS, "rows in LDS");
    constexpr int G = 16, NK = (P + 15) / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int gl = threadIdx.x % G, r = threadIdx.x & 15;
    int64_t chain = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool live = chain < a.C;
    if (!live) chain = a.C - 1;  // whole waves stay converged for the DPP exchanges; stores are masked
    const auto rows = make_rows<T, P, G, MODE, R>(m, gl, reinterpret_cast<T*>(smem_raw));
    T* const ck = reinterpret_cast<T*>(smem_raw) + m.n * (P + kLdsRowPad<T>) + threadIdx.x;  // [2 max_depth NK][256]
    const uint64_t gchain = (uint64_t)(a.chain_offset + chain);
    const int gbase = (int)(threadIdx.x & 63) - gl;  // first lane of the chain's row in the wave

    T x[NK], civ[NK];
    Metric metric;
    metric.load(a, r, reinterpret_cast<T*>(smem_raw) + m.n * (P + kLdsRowPad<T>) + (size_t)2 * a.max_depth * NK * 256);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int j = r + 16 * k, js = j < P ? j : 0;
        x[k] = j < a.p ? a.state[chain * a.p + j] : T(0);
        civ[k] = j < P ? m.prior.inv_var[js] : T(0);
    }
    const double lprior_const = m.prior.lprior_const;
    auto row_sum = [&](T v) { return group_sum<16>(v); };

    // lpost (replicated) and the lane's coordinates of its gradient at the distributed point xo
    auto evaluate = [&](const T (&xo)[NK], T (&go)[NK]) -> double {
        T xb[P], gb[P];
        if constexpr (P >= 16) {
#pragma unroll
            for (int k = 0; k < NK; ++k) dist_gather16<T, P>(xo[k], k, xb);
        } else {
            nuts_gather_small<T, P>(xo[0], xb);
        }
        Prior<T, P> none;
#pragma unroll
        for (int j = 0; j < P; ++j) none.inv_var[j] = T(0);
        none.lprior_const = 0.0;
        double ll = 0, lpr_unused = 0;
        eval_lpost<T, P, G, true, true>(rows, none, xb, gb, ll, lpr_unused);
        if constexpr (P >= 16) {
            go[0] = dist_pick16<T, P, 0>(gb, r);
            if constexpr (NK > 1) go[NK - 1] = dist_pick16<T, P, NK - 1>(gb, r);
        } else {
            T g16[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) g16[j] = j < P ? gb[j < P ? j : 0] : T(0);
            go[0] = dist_pick16<T, 16, 0>(g16, r);
        }
        T qd = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            go[k] = fma_t(-xo[k], civ[k], go[k]);  // + prior
            qd = fma_t(xo[k] * xo[k], civ[k], qd);
        }
        return ll + (lprior_const - 0.5 * (double)row_sum(qd));
    };
    auto turning = [&](const T (&pa)[NK], const T (&pb)[NK], const T (&rh)[NK]) -> bool { return metric.turning(pa, pb, rh); };
    auto kinetic2 = [&](const T (&pm)[NK]) -> double { return metric.kinetic2(pm); };

    T g[NK];
    double lp = evaluate(x, g);
    uint64_t n_leap = 0, depth_sum = 0;
    double acc_sum = 0.0;
    uint32_t n_div = 0, n_hit = 0;
    const int md = a.max_depth;
    const int nsteps = (1 << md) - 1;
    T step;
    if constexpr (TUNED) step = a.tune->step;
    else step = a.step;
    const T heps = T(0.5) * step;
    [[maybe_unused]] double last_stat = 0.0;  // (TUNED) the acceptance statistic of the last iteration
    const int rz = r < P ? r : 0;  // lanes beyond the padded width read coordinate 0's normal (times a zero scale)

    DrawBatch<T, P, G> draws;
    static_assert(DrawBatch<T, P, G>::kEnabled, "batched draws");
    draws.reset();
    for (int64_t it = 0; it < a.iters; ++it) {
        int depth_signed = 0;
        for (int64_t jt = 0; jt < a.thin; ++jt) {
            const uint64_t iter = (uint64_t)(a.iter_offset + it * a.thin + jt);
            T z[NK], lu_unused;
            draws.template next_own<NK>(a.seed, gchain, iter, gl, rz, z, lu_unused);
            // tree blocks: lane r of the row holds doubling r's block (r < max_depth <= 10 are read)
            const U4 tw = philox4x32_10((uint32_t)gchain, (uint32_t)iter, (uint32_t)(iter >> 32), TAG_NUTS_TREE | (uint32_t)r, (uint32_t)a.seed,
                                        (uint32_t)(a.seed >> 32));

            T Lq[NK], Lp[NK], Lg[NK], Rq[NK], Rp[NK], Rg[NK], cq[NK], cp[NK], cg[NK];
            T rho[NK], rhos[NK], pfirst[NK], pinner[NK], px[NK], pg[NK], sx[NK], sg[NK], p0[NK];
            metric.momentum(z, p0);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                Lq[k] = Rq[k] = px[k] = sx[k] = x[k];
                Lg[k] = Rg[k] = pg[k] = sg[k] = g[k];
                Lp[k] = Rp[k] = rho[k] = p0[k];
                rhos[k] = pfirst[k] = T(0);
            }
            double plp = lp, slp = lp;
            const double H0 = 0.5 * kinetic2(Lp) - lp;
            double W = 0.0, Ws = 0.0, sumacc = 0.0;
            int d = 0, i = 0, depth = 0, nleaf = 0;
            bool done = false, div = false, turned = false;
            bool fwd = (lane_word(tw.x, gbase) >> 31) != 0;
            double umerge = u01<double>(lane_word(tw.y, gbase));
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                cq[k] = fwd ? Rq[k] : Lq[k];
                cp[k] = fwd ? Rp[k] : Lp[k];
                cg[k] = fwd ? Rg[k] : Lg[k];
                pinner[k] = cp[k];
            }
            U4 lw4 = {0, 0, 0, 0};
            for (int s = 0; s < nsteps; ++s) {
                if (__builtin_amdgcn_ballot_w64(!done) == 0) break;  // wave-uniform: no chain of the wave is building
                if ((s & 63) == 0)  // leaf uniforms of steps s .. s + 63: lane r holds block s / 4 + r
                    lw4 = philox4x32_10((uint32_t)gchain, (uint32_t)iter, (uint32_t)(iter >> 32), TAG_NUTS_LEAF | (uint32_t)((s >> 2) + r),
                                        (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
                const int w = s & 3;
                const uint32_t wmine = w == 0 ? lw4.x : (w == 1 ? lw4.y : (w == 2 ? lw4.z : lw4.w));
                const double uleaf = u01<double>(lane_word(wmine, gbase + ((s >> 2) & 15)));

                // leapfrog from the moving end, step +-eps
                const T hs = fwd ? heps : -heps;
#pragma unroll
                for (int k = 0; k < NK; ++k) cp[k] = fma_t(hs, cg[k], cp[k]);
                metric.drift(fwd, step, cp, cq);
                const double lpl = evaluate(cq, cg);
#pragma unroll
                for (int k = 0; k < NK; ++k) cp[k] = fma_t(hs, cg[k], cp[k]);
                const double delta = (0.5 * kinetic2(cp) - lpl) - H0;
                const bool ldiv = !(fabs(delta) < __builtin_inf()) || delta > 1000.0;
                const bool act = !done && !ldiv;  // this chain takes the leaf
                const double accl = ldiv ? 0.0 : (delta <= 0.0 ? 1.0 : exp(-delta));
                nleaf += done ? 0 : 1;
                sumacc += done ? 0.0 : accl;
                // uniform progressive sampling inside the subtree
                const double lw = -delta;
                const bool first = i == 0;
                const double Wn = first ? lw : nuts_lae(Ws, lw);
                const bool take = act && (first || uleaf < exp(lw - Wn));
                T rhn[NK];
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    rhn[k] = rhos[k] + cp[k];
                    rhos[k] = act ? rhn[k] : rhos[k];
                    sx[k] = take ? cq[k] : sx[k];
                    sg[k] = take ? cg[k] : sg[k];
                    pfirst[k] = act && first ? cp[k] : pfirst[k];
                }
                slp = take ? lpl : slp;
                Ws = act ? Wn : Ws;
                // checkpoints: an even leaf stores (p, rho) at popcount(i >> 1); an odd one checks the subtrees it closes
                const int idx_max = __builtin_popcount((unsigned)i >> 1);
                const int idx_min = idx_max - __builtin_ctz(~(unsigned)i) + 1;
                const bool even = (i & 1) == 0;
                if (act && even) {
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        ck[((idx_max * 2 + 0) * NK + k) * 256] = cp[k];
                        ck[((idx_max * 2 + 1) * NK + k) * 256] = rhn[k];
                    }
                }
                bool sturn = false;
                for (int j = 0; j < md; ++j) {
                    const bool want = act && !even && j >= idx_min && j <= idx_max;
                    if (__builtin_amdgcn_ballot_w64(want) == 0) continue;  // wave-uniform
                    T kp[NK], kr[NK];
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        kp[k] = ck[((j * 2 + 0) * NK + k) * 256];
                        kr[k] = rhn[k] - ck[((j * 2 + 1) * NK + k) * 256] + kp[k];
                    }
                    const bool t = turning(kp, cp, kr);
                    sturn = sturn || (want && t);
                }
                // end of the subtree: merge it, or end the tree
                const bool end_sub = !done && (ldiv || sturn || i == (1 << d) - 1);
                const bool merge = end_sub && !ldiv && !sturn;
                div = div || (!done && ldiv);
                const bool mtake = merge && umerge < exp(Ws - W);
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    px[k] = mtake ? sx[k] : px[k];
                    pg[k] = mtake ? sg[k] : pg[k];
                }
                plp = mtake ? slp : plp;
                W = merge ? nuts_lae(W, Ws) : W;
                bool tturn = false;
                if (__builtin_amdgcn_ballot_w64(merge) != 0) {  // wave-uniform: the criterion on the whole tree and across the merge
                    T nL[NK], nR[NK], rn[NK], t2[NK], t3[NK], pout[NK];
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        pout[k] = fwd ? Lp[k] : Rp[k];
                        nL[k] = fwd ? Lp[k] : cp[k];
                        nR[k] = fwd ? cp[k] : Rp[k];
                        rn[k] = rho[k] + rhos[k];
                        t2[k] = rho[k] + pfirst[k];
                        t3[k] = rhos[k] + pinner[k];
                    }
                    const bool a1 = turning(nL, nR, rn), a2 = turning(pout, pfirst, t2), a3 = turning(cp, pinner, t3);
                    tturn = merge && (a1 || a2 || a3);
                }
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    rho[k] = merge ? rho[k] + rhos[k] : rho[k];
                    Rq[k] = merge && fwd ? cq[k] : Rq[k];
                    Rp[k] = merge && fwd ? cp[k] : Rp[k];
                    Rg[k] = merge && fwd ? cg[k] : Rg[k];
                    Lq[k] = merge && !fwd ? cq[k] : Lq[k];
                    Lp[k] = merge && !fwd ? cp[k] : Lp[k];
                    Lg[k] = merge && !fwd ? cg[k] : Lg[k];
                }
                depth = end_sub ? d + 1 : depth;
                const bool fin = end_sub && (ldiv || sturn || tturn || d + 1 == md);
                turned = turned || (end_sub && (sturn || tturn));
                const bool next = end_sub && !fin;
                done = done || fin;
                d = next ? d + 1 : d;
                i = next ? 0 : i + 1;
                // the next doubling's direction and merge uniform (read by every lane; used by the chains that go on)
                const bool nfwd = (lane_word(tw.x, gbase + d) >> 31) != 0;
                const double nu = u01<double>(lane_word(tw.y, gbase + d));
                fwd = next ? nfwd : fwd;
                umerge = next ? nu : umerge;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    cq[k] = next ? (nfwd ? Rq[k] : Lq[k]) : cq[k];
                    cp[k] = next ? (nfwd ? Rp[k] : Lp[k]) : cp[k];
                    cg[k] = next ? (nfwd ? Rg[k] : Lg[k]) : cg[k];
                    pinner[k] = next ? cp[k] : pinner[k];
                    rhos[k] = next ? T(0) : rhos[k];
                }
            }
            if (!done) depth = md;  // (unreachable: the step bound is the full tree)
            const bool hit = !div && !turned && depth == md;
            n_leap += (uint64_t)nleaf;
            depth_sum += (uint64_t)depth;
            const double stat = sumacc / (double)(nleaf > 0 ? nleaf : 1);
            acc_sum += stat;
            if constexpr (TUNED) last_stat = stat;
            n_div += div ? 1u : 0u;
            n_hit += hit ? 1u : 0u;
            depth_signed = div ? -depth : depth;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                x[k] = px[k];
                g[k] = pg[k];
            }
            lp = plp;
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int j = r + 16 * k;
                if (j < a.p) {
                    if (a.out) a.out[(it * a.C + chain) * a.p + j] = x[k];
                    if (a.stats.buf) {  // (stats_update of lr_device.h for one coordinate)
                        const int64_t idx = a.stats.first + it, b = idx / a.stats.batch, kk = idx - b * a.stats.batch;
                        double* sbuf = a.stats.buf + ((b * a.C + chain) * 2) * a.p;
                        stats_fold(sbuf + j, sbuf + a.p + j, kk, 1.0 / (double)(kk + 1), (double)x[k]);
                    }
                }
            }
            if (a.depth_out && r == 0) a.depth_out[it * a.C + chain] = (int8_t)depth_signed;
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (r + 16 * k < a.p) a.state[chain * a.p + r + 16 * k] = x[k];
        if (r == 0 && a.counters) {
            NutsCounters* cn = a.counters + chain;
            cn->n_leapfrog += n_leap;
            cn->depth_sum += depth_sum;
            cn->accept_stat_sum += acc_sum;
            cn->divergent += n_div;
            cn->max_depth_hits += n_hit;
        }
        if constexpr (TUNED)
            if (r == 0) a.astat[chain] = last_stat;
    }
}

template <typename T, int P, int MODE, int R, bool TUNED = false>
__global__ void __launch_bounds__(256) k_nuts(ModelArgs<T, P> m, NutsArgsOf<T, P, TUNED> a) {
    nuts_run<T, P, MODE, R, TUNED, NutsDiagMetric<T, P, TUNED>>(m, a);
}

}  // namespace lr
