// lr_tall_nuts_update.inc -- the body of k_tall_nuts_update and k_tall_nuts_update_tuned (lr_tall_nuts.h), included once in each with
// `constexpr bool TUNED` set: one text, two kernels.  (A shared device function was tried: with the arguments handed on, by value or by
// reference, the plain kernel no longer compiled to the code it had; as a template flag on one kernel the plain kernel's symbol changes,
// which the recorded launch traces name.)  In scope: T, P, TUNED; the kernel's parameters a, n, phase, iter, s, d, i, out_row, flag.
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t chain = gt / P;
    const int j = (int)(gt % P);
    const bool live = chain < a.C;
    if (!live) chain = a.C - 1;  // whole blocks stay converged for chain_sum; stores are masked
    const int64_t ix = chain * P + j, CP = a.C * P;
    const uint64_t gchain = (uint64_t)(a.chain_offset + chain);
    const auto& tn = [&]() -> const auto& {  // where step, a, b, c come from
        if constexpr (TUNED) return *n.tune;
        else return a;
    }();
    const T aj = tn.a[j], bj = tn.b[j], cj = tn.c[j], ivj = a.prior.inv_var[j];
    const T heps = T(0.5) * tn.step;
    // a chain's scalars: one record per wave of the chain (P > 64: two), each read and written by that wave alone -- every lane computes
    // the same values, so the copies are equal and no wave reads what another writes
    NutsTallChain* const ch = n.ch + chain * nuts_tall_waves_per_chain(P) + (j >> 6);
    const bool writer = (j & 63) == 0;  // the lane that keeps the wave's record
    auto V = [&](int k) -> T& { return n.v[(int64_t)k * CP + ix]; };
    auto tree_word = [&](uint64_t it, int dd) {  // doubling dd: word x bit 31 = direction, word y = merge uniform
        return philox4x32_10((uint32_t)gchain, (uint32_t)it, (uint32_t)(it >> 32), TAG_NUTS_TREE | (uint32_t)dd, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    };
    auto kinetic2 = [&](T pm) { return (double)chain_sum<P>(pm * pm * cj); };  // sum p^2 / dmm
    // generalised U-turn criterion (NutsDiagMetric::turning of lr_nuts.h)
    auto turning = [&](T pa, T pb, T rh) {
        const T rr = fma_t(T(-0.5), pa + pb, rh);
        const T sa = chain_sum<P>(cj * pa * rr), sb = chain_sum<P>(cj * pb * rr);
        return sa <= T(0) || sb <= T(0);
    };
    // start iteration `it` from (x, g, lp)
    auto begin = [&](uint64_t it, T x, T g, double lp, bool first_of_call) {
        const T p0 = tall_normal_j<T>(a.seed, gchain, it, j) * aj;
        const double H0 = 0.5 * kinetic2(p0) - lp;
        const U4 tw = tree_word(it, 0);
        const bool fwd = (tw.x >> 31) != 0;
        const T cp = fma_t(fwd ? heps : -heps, g, p0);
        if (live) {
            V(NTV_LQ) = V(NTV_RQ) = V(NTV_PX) = V(NTV_SX) = x;
            V(NTV_LG) = V(NTV_RG) = V(NTV_PG) = V(NTV_SG) = g;
            V(NTV_LP) = V(NTV_RP) = V(NTV_RHO) = V(NTV_PINNER) = p0;
            V(NTV_RHOS) = V(NTV_PFIRST) = T(0);
            V(NTV_CP) = cp;
            a.q1[ix] = fma_t(fwd ? bj : -bj, cp, x);
            if (writer) {
                ch->lp = ch->plp = ch->slp = lp;
                ch->H0 = H0;
                ch->W = ch->Ws = ch->sumacc = 0.0;
                ch->umerge = u01<double>(tw.y);
                ch->nleaf = ch->depth = 0;
                ch->flags = fwd ? NTF_FWD : 0;
                if (first_of_call) {
                    // (TUNED: the sum goes on from the caller's, so that it does not depend on how a warm-up was cut into calls)
                    if constexpr (TUNED) ch->acc_sum = n.counters ? n.counters[chain].accept_stat_sum : 0.0;
                    else ch->acc_sum = 0.0;
                    ch->n_leap = ch->depth_sum = 0;
                    ch->n_div = ch->n_hit = 0;
                }
            }
        }
        if (gt < kNutsTallSlots) n.tally[gt] = 0;
    };

    if (phase == NPH_BEGIN) {  // after the evaluation at x (= q1)
        const T g = tall_reduced_grad<T, P>(a, chain, j, ivj);
        const double lp = tall_reduced_value<T, P>(a, chain, j, ivj);
        if (live) a.g[ix] = g;
        begin((uint64_t)iter, a.x[ix], g, lp, true);
        return;
    }
    if constexpr (TUNED) {
        if (phase == NPH_CARRY) {  // what NPH_END does with flag = 1, after the tuning block was rewritten
            begin((uint64_t)iter, a.x[ix], a.g[ix], ch->lp, false);
            return;
        }
    }
    if (phase == NPH_LEAF) {
        const int flags = ch->flags;
        const bool done = (flags & NTF_DONE) != 0, fwd = (flags & NTF_FWD) != 0;
        const double H0 = ch->H0, W0 = ch->W, Ws0 = ch->Ws, umerge = ch->umerge;
        // ---- after `evaluate` for leaf s
        T cg = tall_reduced_grad<T, P>(a, chain, j, ivj);
        const double lpl = tall_reduced_value<T, P>(a, chain, j, ivj);
        T cq = a.q1[ix];
        T cp = fma_t(fwd ? heps : -heps, cg, V(NTV_CP));
        const double delta = (0.5 * kinetic2(cp) - lpl) - H0;
        const bool ldiv = !(fabs(delta) < __builtin_inf()) || delta > 1000.0;
        const bool act = !done && !ldiv;  // this chain takes the leaf
        const double accl = ldiv ? 0.0 : (delta <= 0.0 ? 1.0 : exp(-delta));
        // uniform progressive sampling inside the subtree
        const U4 lw4 = philox4x32_10((uint32_t)gchain, (uint32_t)iter, (uint32_t)((uint64_t)iter >> 32), TAG_NUTS_LEAF | (uint32_t)(s >> 2), (uint32_t)a.seed,
                                     (uint32_t)(a.seed >> 32));
        const int w = s & 3;
        const double uleaf = u01<double>(w == 0 ? lw4.x : (w == 1 ? lw4.y : (w == 2 ? lw4.z : lw4.w)));
        const double lw = -delta;
        const bool first = i == 0;
        const double Wn = first ? lw : nuts_lae(Ws0, lw);
        const bool take = act && (first || uleaf < exp(lw - Wn));
        const T rhos0 = V(NTV_RHOS);
        const T rhn = rhos0 + cp;
        T rhos = act ? rhn : rhos0;
        const double Ws = act ? Wn : Ws0;
        // checkpoints: an even leaf stores (p, rho) at popcount(i >> 1); an odd one checks the subtrees it closes
        const int idx_max = __builtin_popcount((unsigned)i >> 1);
        const int idx_min = idx_max - __builtin_ctz(~(unsigned)i) + 1;
        const bool even = (i & 1) == 0;
        bool sturn = false;
        if (even) {
            if (live && act) {
                V(NTV_COUNT + 2 * idx_max) = cp;
                V(NTV_COUNT + 2 * idx_max + 1) = rhn;
            }
        } else {
            for (int k = idx_min; k <= idx_max; ++k) {  // uniform over the launch
                const T kp = V(NTV_COUNT + 2 * k);
                const T kr = rhn - V(NTV_COUNT + 2 * k + 1) + kp;
                const bool t = turning(kp, cp, kr);
                sturn = sturn || (act && t);
            }
        }
        // end of the subtree: merge it, or end the tree
        const bool last = i == (1 << d) - 1;  // uniform: a merge and a next doubling happen at this leaf only
        const bool end_sub = !done && (ldiv || sturn || last);
        const bool merge = end_sub && !ldiv && !sturn;
        const bool mtake = merge && umerge < exp(Ws - W0);
        const double W = merge ? nuts_lae(W0, Ws) : W0;
        bool tturn = false;
        T rho = T(0);
        if (last) {  // the criterion on the whole tree and across the merge
            rho = V(NTV_RHO);
            const T pinner = V(NTV_PINNER), pfirst = act && first ? cp : V(NTV_PFIRST);
            const T pout = fwd ? V(NTV_LP) : V(NTV_RP);
            const bool a1 = turning(fwd ? pout : cp, fwd ? cp : pout, rho + rhos);
            const bool a2 = turning(pout, pfirst, rho + pfirst);
            const bool a3 = turning(cp, pinner, rhos + pinner);
            tturn = merge && (a1 || a2 || a3);
        }
        const int md = n.max_depth;
        const bool fin = end_sub && (ldiv || sturn || tturn || d + 1 == md);
        const bool next = end_sub && !fin;
        const bool done_after = done || fin;
        // ---- stores of the leaf (a finished chain: none)
        if (live && take) {
            V(NTV_SX) = cq;
            V(NTV_SG) = cg;
        }
        if (live && act && first) V(NTV_PFIRST) = cp;
        if (live && mtake) {
            V(NTV_PX) = take ? cq : V(NTV_SX);
            V(NTV_PG) = take ? cg : V(NTV_SG);
        }
        if (live && merge) {
            V(NTV_RHO) = rho + rhos;
            V(fwd ? NTV_RQ : NTV_LQ) = cq;
            V(fwd ? NTV_RP : NTV_LP) = cp;
            V(fwd ? NTV_RG : NTV_LG) = cg;
        }
        // ---- before `evaluate` for leaf s + 1: the next doubling's direction and merge uniform, the new moving end
        bool nfwd = fwd;
        double nu = umerge;
        if (next) {  // (per chain; no sum inside)
            const U4 tw = tree_word((uint64_t)iter, d + 1);
            nfwd = (tw.x >> 31) != 0;
            nu = u01<double>(tw.y);
            if (nfwd != fwd) {  // the other end of the tree (the merge above left it as it was)
                cq = V(nfwd ? NTV_RQ : NTV_LQ);
                cp = V(nfwd ? NTV_RP : NTV_LP);
                cg = V(nfwd ? NTV_RG : NTV_LG);
            }
            rhos = T(0);
            if (live) V(NTV_PINNER) = cp;
        }
        if (live && !done_after) {
            V(NTV_RHOS) = rhos;
            cp = fma_t(nfwd ? heps : -heps, cg, cp);
            V(NTV_CP) = cp;
            a.q1[ix] = fma_t(nfwd ? bj : -bj, cp, cq);
        }
        if (live && !done && writer) {
            ch->nleaf += 1;
            ch->sumacc += accl;
            if (take) ch->slp = lpl;
            if (mtake) ch->plp = take ? lpl : ch->slp;
            ch->Ws = Ws;
            ch->W = W;
            ch->umerge = nu;
            if (end_sub) ch->depth = d + 1;
            ch->flags = (done_after ? NTF_DONE : 0) | ((flags & NTF_DIV) || ldiv ? NTF_DIV : 0) |
                        ((flags & NTF_TURNED) || (end_sub && (sturn || tturn)) ? NTF_TURNED : 0) | (nfwd ? NTF_FWD : 0);
        }
        if (flag && live && j == 0 && !done_after) atomicAdd(&n.tally[d], 1u);  // an integer tally for the host's early stop; it feeds no arithmetic
        return;
    }
    if (phase == NPH_END) {
        const int flags = ch->flags, md = n.max_depth;
        const bool div = (flags & NTF_DIV) != 0, turned = (flags & NTF_TURNED) != 0;
        const int depth = (flags & NTF_DONE) ? ch->depth : md;  // (not done: the step bound is the full tree)
        const int nleaf = ch->nleaf;
        const double sumacc = ch->sumacc, lp = ch->plp;
        const T x = V(NTV_PX), g = V(NTV_PG);
        const bool hit = !div && !turned && depth == md;
        const int depth_signed = div ? -depth : depth;
        if (live) {
            a.x[ix] = x;
            a.g[ix] = g;
            if (writer) {
                ch->n_leap += (uint64_t)nleaf;
                ch->depth_sum += (uint64_t)depth;
                ch->acc_sum += sumacc / (double)(nleaf > 0 ? nleaf : 1);
                ch->n_div += div ? 1u : 0u;
                ch->n_hit += hit ? 1u : 0u;
            }
            if (out_row >= 0 && j < a.p) {
                if (a.out) a.out[(out_row * a.C + chain) * a.p + j] = x;
                if (a.stats.buf) {  // lane = coordinate: one (mean, M2) pair each
                    const int64_t idx = a.stats.first + out_row, sb = idx / a.stats.batch, sk = idx - sb * a.stats.batch;
                    double* sbuf = a.stats.buf + ((sb * a.C + chain) * 2) * a.p;
                    stats_fold(sbuf + j, sbuf + a.p + j, sk, 1.0 / (double)(sk + 1), (double)x);
                }
            }
            if (out_row >= 0 && j == 0 && n.depth_out) n.depth_out[out_row * a.C + chain] = (int8_t)depth_signed;
            if constexpr (TUNED)
                if (j == 0) n.astat[chain] = sumacc / (double)(nleaf > 0 ? nleaf : 1);
        }
        if (flag) begin((uint64_t)iter + 1, x, g, lp, false);
        else if (live && writer) ch->lp = lp;
        return;
    }
    if (phase == NPH_STORE) {
        if (live) {
            if (j < a.p) a.state[chain * a.p + j] = a.x[ix];
            if (j == 0 && n.counters) {
                NutsCounters* cn = n.counters + chain;
                cn->n_leapfrog += ch->n_leap;
                cn->depth_sum += ch->depth_sum;
                if constexpr (TUNED) cn->accept_stat_sum = ch->acc_sum;
                else cn->accept_stat_sum += ch->acc_sum;
                cn->divergent += ch->n_div;
                cn->max_depth_hits += ch->n_hit;
            }
        }
    }
