/*
 * lr_cpu_twin_nuts.c -- the CPU TEST DOUBLE of include/logreg_hip_nuts.h: the whole ABI of lr_cpu_twin.c plus lr_run_nuts, in float64
 * on the oracle's model functions and Philox stream.  TEST INFRASTRUCTURE ONLY (tests/twin_nuts.py builds and injects it).
 *
 * It follows DESIGN.md "NUTS" decision by decision, in the order written there: it is the step-parity reference of the kernel
 * (logreg_amd/csrc/lr_nuts.h) and the double the Python face is tested against.  Every multiply-add the kernel fuses is an fma()
 * here, so that a float64 model agrees with the device up to the summation order of its sums.
 */
/* the base double's planner knows kinds 0..3: its entry points are renamed and wrapped below */
#define lr_plan_run twin_base_plan_run
#define lr_plan_run_info twin_base_plan_run_info
#include "lr_cpu_twin.c"
#undef lr_plan_run
#undef lr_plan_run_info

#include "../../include/logreg_hip_nuts.h"

LR_API int lr_plan_run(const lr_model *m, int32_t kind, const lr_run_opts *o, int32_t *mode_out, int32_t *group_out, int32_t *rows_out) {
    int rc = check_opts(m, o, 0);
    if (rc) return rc;
    if (kind < LR_KIND_RWMH || kind > LR_KIND_NUTS) return fail(LR_ERR_INVALID, "unknown kernel family %d", kind);
    if (kind == LR_KIND_NUTS && m->p > 32) return fail(LR_ERR_UNSUPPORTED, "NUTS: p = %d > 32 has no resident-row kernel", m->p);
    return lr_plan(m, o->plan_chains > 0 ? o->plan_chains : o->n_chains, o->group, o->mode, mode_out, group_out, rows_out);
}
LR_API int lr_plan_run_info(const lr_model *m, int32_t kind, const lr_run_opts *opts, lr_plan_info *out) {
    if (!out) return fail(LR_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof *out);
    return lr_plan_run(m, kind, opts, &out->mode, &out->group, &out->rows);
}

static double nuts_lae(double a, double b) { /* log(exp(a) + exp(b)), both finite */
    const double mx = a > b ? a : b, d = a > b ? b - a : a - b;
    return mx + log1p(exp(d));
}
/* turning(a, b, rho): rho' = rho - (a + b) / 2; (a/dmm) . rho' <= 0 or (b/dmm) . rho' <= 0 */
static int nuts_turning(const double *c, const double *a, const double *b, const double *rho, int p) {
    double sa = 0.0, sb = 0.0;
    for (int j = 0; j < p; ++j) {
        const double r = fma(-0.5, a[j] + b[j], rho[j]);
        sa = fma(c[j] * a[j], r, sa);
        sb = fma(c[j] * b[j], r, sb);
    }
    return sa <= 0.0 || sb <= 0.0;
}
static double nuts_kin(const double *c, const double *p, int n) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s = fma(p[j] * p[j], c[j], s);
    return s;
}

#define NUTS_MAXP 32 /* the kernel's widest padded width */
typedef struct { double q[NUTS_MAXP], p[NUTS_MAXP], g[NUTS_MAXP]; } nuts_pt;

/* one NUTS iteration of one chain (DESIGN.md "NUTS"); x, g, lp in/out */
static void nuts_iteration(const orc_model *om, const double *sqd, const double *b, const double *c, double eps, int max_depth, uint64_t seed,
                           uint64_t chain, uint64_t iter, double *x, double *g, double *lp, lr_nuts_counters *cnt, int *depth_signed) {
    const int p = om->p;
    double z[NUTS_MAXP];
    orc_draws(seed, chain, iter, p, z, NULL);
    nuts_pt L = {{0}, {0}, {0}}, R, cur;
    double rho[NUTS_MAXP], rhos[NUTS_MAXP], rho_old[NUTS_MAXP], pfirst[NUTS_MAXP], pinner[NUTS_MAXP], tmp[NUTS_MAXP];
    double ck_p[LR_NUTS_MAX_DEPTH][NUTS_MAXP], ck_r[LR_NUTS_MAX_DEPTH][NUTS_MAXP];
    double prop_x[NUTS_MAXP], prop_g[NUTS_MAXP], prop_lp = *lp, sub_x[NUTS_MAXP], sub_g[NUTS_MAXP], sub_lp = 0.0;
    for (int j = 0; j < p; ++j) {
        L.q[j] = x[j];
        L.p[j] = z[j] * sqd[j];
        L.g[j] = g[j];
        rho[j] = L.p[j];
        prop_x[j] = x[j];
        prop_g[j] = g[j];
    }
    R = L;
    const double H0 = 0.5 * nuts_kin(c, L.p, p) - *lp;
    double W = 0.0, sumacc = 0.0;
    uint64_t nleaf = 0;
    int depth = 0, div = 0, turned = 0;
    const double heps = 0.5 * eps;
    for (int d = 0; d < max_depth && !div && !turned; ++d) {
        uint32_t wt[4];
        stream_block(seed, chain, iter, LR_NUTS_TAG_TREE | (uint32_t)d, wt);
        const int fwd = (wt[0] >> 31) != 0;
        const double sgn = fwd ? 1.0 : -1.0, umerge = u01(wt[1]);
        cur = fwd ? R : L;
        memcpy(pinner, cur.p, sizeof(double) * p);
        double Ws = 0.0;
        for (int j = 0; j < p; ++j) rhos[j] = 0.0;
        const int64_t nsub = (int64_t)1 << d;
        for (int64_t i = 0; i < nsub; ++i) {
            const uint64_t k = nleaf;
            /* leapfrog, step sgn * eps */
            for (int j = 0; j < p; ++j) cur.p[j] = fma(sgn * heps, cur.g[j], cur.p[j]);
            for (int j = 0; j < p; ++j) cur.q[j] = fma(sgn * b[j], cur.p[j], cur.q[j]);
            const double lpl = orc_lpost(om, cur.q);
            orc_glp(om, cur.q, cur.g);
            for (int j = 0; j < p; ++j) cur.p[j] = fma(sgn * heps, cur.g[j], cur.p[j]);
            ++nleaf;
            const double H = 0.5 * nuts_kin(c, cur.p, p) - lpl, delta = H - H0;
            const int ldiv = !(fabs(delta) < INFINITY) || delta > 1000.0;
            if (!ldiv) sumacc += delta <= 0.0 ? 1.0 : exp(-delta);
            if (ldiv) {
                div = 1;
                break;
            }
            const double lw = -delta;
            for (int j = 0; j < p; ++j) rhos[j] += cur.p[j];
            if (i == 0) {
                Ws = lw;
                memcpy(sub_x, cur.q, sizeof(double) * p);
                memcpy(sub_g, cur.g, sizeof(double) * p);
                sub_lp = lpl;
                memcpy(pfirst, cur.p, sizeof(double) * p);
            } else {
                const double Wn = nuts_lae(Ws, lw);
                uint32_t wl[4];
                stream_block(seed, chain, iter, LR_NUTS_TAG_LEAF | (uint32_t)(k / 4), wl);
                if (u01(wl[k % 4]) < exp(lw - Wn)) {
                    memcpy(sub_x, cur.q, sizeof(double) * p);
                    memcpy(sub_g, cur.g, sizeof(double) * p);
                    sub_lp = lpl;
                }
                Ws = Wn;
            }
            const int idx_max = __builtin_popcountll((uint64_t)i >> 1);
            if ((i & 1) == 0) {
                memcpy(ck_p[idx_max], cur.p, sizeof(double) * p);
                memcpy(ck_r[idx_max], rhos, sizeof(double) * p);
            } else {
                const int idx_min = idx_max - __builtin_ctzll(~(uint64_t)i) + 1;
                for (int jj = idx_max; jj >= idx_min && !turned; --jj) {
                    for (int j = 0; j < p; ++j) tmp[j] = rhos[j] - ck_r[jj][j] + ck_p[jj][j];
                    turned = nuts_turning(c, ck_p[jj], cur.p, tmp, p);
                }
                if (turned) break;
            }
        }
        depth = d + 1;
        if (div || turned) break;
        /* merge: biased progressive sampling, then the U-turn criterion on the whole tree and across the merge */
        if (umerge < exp(Ws - W)) {
            memcpy(prop_x, sub_x, sizeof(double) * p);
            memcpy(prop_g, sub_g, sizeof(double) * p);
            prop_lp = sub_lp;
        }
        W = nuts_lae(W, Ws);
        for (int j = 0; j < p; ++j) {
            rho_old[j] = rho[j];
            rho[j] += rhos[j];
        }
        const double *pouter_old = fwd ? L.p : R.p;
        int t = 0;
        if (fwd) R = cur;
        else L = cur;
        t = nuts_turning(c, L.p, R.p, rho, p);
        for (int j = 0; j < p; ++j) tmp[j] = rho_old[j] + pfirst[j];
        t = t || nuts_turning(c, pouter_old, pfirst, tmp, p);
        for (int j = 0; j < p; ++j) tmp[j] = rhos[j] + pinner[j];
        t = t || nuts_turning(c, cur.p, pinner, tmp, p);
        turned = t;
    }
    const int hit = !div && !turned && depth == max_depth;
    cnt->n_leapfrog += nleaf;
    cnt->depth_sum += (uint64_t)depth;
    cnt->accept_stat_sum += sumacc / (double)nleaf;
    cnt->divergent += (uint32_t)div;
    cnt->max_depth_hits += (uint32_t)hit;
    *depth_signed = div ? -depth : depth;
    memcpy(x, prop_x, sizeof(double) * p);
    memcpy(g, prop_g, sizeof(double) * p);
    *lp = prop_lp;
}

LR_API int lr_run_nuts(lr_model *m, void *state, double eps, int32_t max_depth, const double *dmm, const lr_run_opts *o, void *out,
                       lr_nuts_counters *counters, int8_t *depth_out) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    int rc = positive_vec("dmm", dmm, m->p);
    if (rc) return rc;
    if (!(eps > 0) || !isfinite(eps)) return fail(LR_ERR_INVALID, "eps must be finite and > 0");
    if (max_depth < 1 || max_depth > LR_NUTS_MAX_DEPTH) return fail(LR_ERR_INVALID, "max_depth must be in 1..%d", LR_NUTS_MAX_DEPTH);
    rc = check_opts(m, o, 1);
    if (rc) return rc;
    if (m->p > 32) return fail(LR_ERR_UNSUPPORTED, "NUTS: p = %d > 32 has no resident-row kernel", m->p);
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    const int p = m->p;
    const int64_t C = o->n_chains;
    double sqd[NUTS_MAXP], b[NUTS_MAXP], c[NUTS_MAXP]; /* sqrt(dmm), eps / dmm, 1 / dmm: the kernel's constants */
    for (int j = 0; j < p; ++j) {
        sqd[j] = sqrt(dmm[j]);
        b[j] = eps / dmm[j];
        c[j] = 1.0 / dmm[j];
    }
    for (int64_t ch = 0; ch < C; ++ch) {
        double x[NUTS_MAXP], g[NUTS_MAXP], lp;
        for (int j = 0; j < p; ++j) x[j] = get(state, m->dtype, ch * p + j);
        lp = orc_lpost(&m->om, x);
        orc_glp(&m->om, x, g);
        lr_nuts_counters cnt = {0, 0, 0.0, 0, 0};
        for (int64_t i = 0; i < o->iters; ++i) {
            int ds = 0;
            for (int64_t t = 0; t < o->thin; ++t)
                nuts_iteration(&m->om, sqd, b, c, eps, max_depth, o->seed, (uint64_t)(o->chain_offset + ch),
                               (uint64_t)(o->iter_offset + i * o->thin + t), x, g, &lp, &cnt, &ds);
            if (m->dtype == LR_F32) { /* the state as the device stores it; value and gradient follow the stored point */
                int changed = 0;
                for (int j = 0; j < p; ++j) {
                    const double r = (double)(float)x[j];
                    changed |= r != x[j];
                    x[j] = r;
                }
                if (changed) {
                    lp = orc_lpost(&m->om, x);
                    orc_glp(&m->om, x, g);
                }
            }
            if (out)
                for (int j = 0; j < p; ++j) put(out, m->dtype, (i * C + ch) * p + j, x[j]);
            if (depth_out) depth_out[i * C + ch] = (int8_t)ds;
            if (o->stats) {
                const int64_t idx = o->stats_first + i, b = idx / o->stats_batch, kk = idx - b * o->stats_batch;
                double *s = o->stats + ((b * C + ch) * 2) * p;
                for (int j = 0; j < p; ++j) {
                    if (kk == 0) {
                        s[j] = x[j];
                        s[p + j] = 0.0;
                    } else {
                        const double dlt = x[j] - s[j];
                        s[j] += dlt / (double)(kk + 1);
                        s[p + j] += dlt * (x[j] - s[j]);
                    }
                }
            }
        }
        for (int j = 0; j < p; ++j) put(state, m->dtype, ch * p + j, x[j]);
        if (counters) {
            counters[ch].n_leapfrog += cnt.n_leapfrog;
            counters[ch].depth_sum += cnt.depth_sum;
            counters[ch].accept_stat_sum += cnt.accept_stat_sum;
            counters[ch].divergent += cnt.divergent;
            counters[ch].max_depth_hits += cnt.max_depth_hits;
        }
    }
    return LR_OK;
}
