/*
 * lr_cpu_twin_hs.c -- the CPU TEST DOUBLE of include/logreg_hip_hs.h: the whole ABI of lr_cpu_twin_pg.c plus lr_run_hs and lr_hs_hyper, in
 * float64 on the oracle's Philox stream.  TEST INFRASTRUCTURE ONLY (tests/twin_hs.py builds and injects it).
 *
 * The beta-step is pg_sweep of lr_cpu_twin_pg.c with the horseshoe's precision on the diagonal; the hyper-step follows the text of
 * include/logreg_hip_hs.h and sums as the kernel (logreg_amd/csrc/lr_hs.h) does: per-lane partial sums, then the 16-lane butterfly.
 */
#include "lr_cpu_twin_pg.c"

#include "../../include/logreg_hip_hs.h"

static double hs_expo(uint32_t wa, uint32_t wb) {
    const double u = (((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) + 0.5) * 0x1p-53;
    return -log(u);
}
static double hs_clamp(double v, double old, uint32_t *n) {
    if (v != v) {
        ++*n;
        return old;
    }
    if (v < LR_HS_MIN || v > LR_HS_MAX) ++*n;
    return v < LR_HS_MIN ? LR_HS_MIN : (v > LR_HS_MAX ? LR_HS_MAX : v);
}
static double hs_sane(double v) {
    uint32_t unused = 0;
    return hs_clamp(v, 1.0, &unused);
}

typedef struct {
    uint8_t shrink[PG_MAXP];
    int m;
    double tau0;
} hs_prior;

/* steps 5-7 of one chain: hin [2p+2] -> hout [2p+2]; returns the clamps */
static uint32_t hs_hyper_step(int p, const hs_prior *pr, uint64_t seed, uint64_t chain, uint64_t iter, const double *beta, const double *hin, double *hout) {
    const double tau2 = hs_sane(hin[2 * p]), xi = hs_sane(hin[2 * p + 1]), half_it2 = 0.5 * (1.0 / tau2);
    double part[16], e[16];
    uint32_t n = 0, w[4];
    for (int r = 0; r < 16; ++r) part[r] = 0.0;
    for (int j = 0; j < p; ++j) {
        const double l_old = hs_sane(hin[j]), n_old = hs_sane(hin[p + j]);
        hout[j] = l_old;
        hout[p + j] = n_old;
        if (!pr->shrink[j]) continue;
        stream_block(seed, chain, iter, LR_HS_TAG | (uint32_t)j, w);
        const double b2 = beta[j] * beta[j];
        const double l_new = hs_clamp((1.0 / n_old + b2 * half_it2) / hs_expo(w[0], w[1]), l_old, &n);
        const double il = 1.0 / l_new;
        hout[j] = l_new;
        hout[p + j] = hs_clamp((1.0 + il) / hs_expo(w[2], w[3]), n_old, &n);
        part[j & 15] += b2 * il;
    }
    const double quad = pg_sum16(part);
    const int nexp = (pr->m + 1) / 2;
    for (int k = 0; k < 16; ++k) {
        stream_block(seed, chain, iter, LR_HS_TAG | (uint32_t)(LR_HS_BLOCK_GAMMA + k / 2), w);
        e[k] = k < nexp ? ((k & 1) ? hs_expo(w[2], w[3]) : hs_expo(w[0], w[1])) : 0.0;
    }
    stream_block(seed, chain, iter, LR_HS_TAG | LR_HS_BLOCK_GLOBAL, w);
    double g = pg_sum16(e);
    if ((pr->m + 1) & 1) {
        const double z = sqrt(-2.0 * log(((double)w[2] + 0.5) * 0x1p-32)) * cos(2.0 * PG_PI * (((double)w[3] + 0.5) * 0x1p-32));
        g += 0.5 * (z * z);
    }
    const double t_new = hs_clamp((1.0 / xi + 0.5 * quad) / g, tau2, &n);
    hout[2 * p] = t_new;
    hout[2 * p + 1] = hs_clamp((1.0 / (pr->tau0 * pr->tau0) + 1.0 / t_new) / hs_expo(w[0], w[1]), xi, &n);
    return n;
}

/* one sweep of one chain, beta and hyper in/out: pg_sweep with the horseshoe's precision, then the hyper-step.  Returns 1 if the chain
 * stayed in place. */
static int hs_sweep(const lr_model *m, const double *bvec, const hs_prior *pr, uint64_t seed, uint64_t chain, uint64_t iter, double *beta, double *hyper, double *psi,
                    double *om, lr_hs_counters *cnt) {
    const int p = m->p;
    if (!pg_psi(m, beta, psi)) return 1;
    uint64_t nprop = 0, nterm = 0;
    for (int64_t i = 0; i < m->n; ++i) om[i] = pg_draw(psi[i], seed, chain, iter, (uint32_t)i, &nprop, &nterm);
    static __thread double A[PG_MAXP][PG_MAXP];
    double d[PG_MAXP], y[PG_MAXP], z[PG_MAXP], x[PG_MAXP];
    for (int j = 0; j < p; ++j)
        for (int c = 0; c < p; ++c) A[j][c] = 0.0;
    for (int64_t i = 0; i < m->n; ++i)
        for (int j = 0; j < p; ++j) {
            const double xj = pg_xs(m, i, j);
            for (int c = 0; c < p; ++c) A[j][c] = fma(om[i], xj * pg_xs(m, i, c), A[j][c]);
        }
    const double it2 = 1.0 / hs_sane(hyper[2 * p]);
    for (int j = 0; j < p; ++j) {
        A[j][j] += 1.0 / (m->sd[j] * m->sd[j]) + (pr->shrink[j] ? 1.0 : 0.0) * (it2 * (1.0 / hs_sane(hyper[j])));
        d[j] = 1.0 / sqrt(A[j][j]);
    }
    for (int j = 0; j < p; ++j)
        for (int c = 0; c < p; ++c) A[j][c] = A[j][c] * (d[j] * d[c]);
    for (int j = 0; j < p; ++j) y[j] = d[j] * bvec[j];
    int ok = 1;
    for (int c = 0; c < p; ++c) {
        const double piv = A[c][c];
        ok = ok && (piv > 0.0) && (piv < INFINITY);
        const double lcc = sqrt(piv);
        for (int j = 0; j < p; ++j) A[j][c] = j == c ? lcc : A[j][c] / lcc;
        const double yc = y[c] / lcc;
        y[c] = yc;
        for (int j = c + 1; j < p; ++j) y[j] = fma(-A[j][c], yc, y[j]);
        for (int c2 = c + 1; c2 < p; ++c2) {
            const double l2 = A[c2][c];
            for (int j = 0; j < p; ++j) A[j][c2] = fma(-A[j][c], l2, A[j][c2]);
        }
    }
    if (!ok) return 1;
    orc_draws(seed, chain, iter, p, z, NULL);
    for (int j = 0; j < p; ++j) x[j] = y[j] + z[j];
    for (int c = p - 1; c >= 0; --c) {
        double part[16];
        for (int r = 0; r < 16; ++r) {
            part[r] = 0.0;
            for (int j = r; j < p; j += 16)
                if (j > c) part[r] = fma(A[j][c], x[j], part[r]);
        }
        x[c] = (x[c] - pg_sum16(part)) / A[c][c];
    }
    for (int j = 0; j < p; ++j) {
        beta[j] = d[j] * x[j];
        if (m->dtype == LR_F32) beta[j] = (double)(float)beta[j]; /* the state as stored */
    }
    double hnew[2 * PG_MAXP + 2];
    cnt->clamped += hs_hyper_step(p, pr, seed, chain, iter, beta, hyper, hnew);
    memcpy(hyper, hnew, sizeof(double) * (size_t)(2 * p + 2));
    cnt->proposals += nprop;
    cnt->series_terms += nterm;
    return 0;
}

/* what both entry points refuse about the prior and the hyper-state (host memory) */
static int hs_check(const char *who, const lr_model *m, const lr_hs_prior *prior, const lr_run_opts *o, const double *hyper, const char *hyper_name, hs_prior *pr) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!prior) return fail(LR_ERR_INVALID, "%s: prior is NULL", who);
    if (!prior->shrink) return fail(LR_ERR_INVALID, "%s: prior->shrink is NULL", who);
    if (!(prior->global_scale > 0) || !isfinite(prior->global_scale)) return fail(LR_ERR_INVALID, "%s: global_scale must be finite and > 0", who);
    if (m->p > 32) return fail(LR_ERR_UNSUPPORTED, "PG: p = %d > 32", m->p);
    pr->m = 0;
    pr->tau0 = prior->global_scale;
    for (int j = 0; j < m->p; ++j) {
        pr->shrink[j] = prior->shrink[j] ? 1 : 0;
        pr->m += pr->shrink[j];
    }
    if (!hyper) return fail(LR_ERR_INVALID, "%s is NULL", hyper_name);
    if (o && !o->on_device && o->n_chains > 0) {
        const size_t w = 2 * (size_t)m->p + 2;
        for (size_t i = 0; i < (size_t)o->n_chains * w; ++i)
            if (!(hyper[i] >= LR_HS_MIN && hyper[i] <= LR_HS_MAX))
                return fail(LR_ERR_INVALID, "%s[%zu][%zu] = %g must be finite and > 0 (in [%g, %g])", hyper_name, i / w, i % w, hyper[i], LR_HS_MIN, LR_HS_MAX);
    }
    return LR_OK;
}

LR_API int lr_run_hs(lr_model *m, const lr_hs_prior *prior, void *state, double *hyper, const lr_run_opts *o, void *out, double *scale_out, lr_hs_counters *counters) {
    hs_prior pr;
    int rc = hs_check("lr_run_hs", m, prior, o, hyper, "hyper", &pr);
    if (rc) return rc;
    if ((rc = pg_check(m, o))) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    const int p = m->p;
    const int64_t C = o->n_chains;
    double bvec[PG_MAXP];
    pg_bvec(m, bvec);
    double *psi = (double *)malloc(sizeof(double) * (size_t)m->n * 2), *om = psi + m->n;
    if (!psi) return fail(LR_ERR_NOMEM, "run scratch");
    for (int64_t ch = 0; ch < C; ++ch) {
        double x[PG_MAXP], *h = hyper + ch * (2 * p + 2);
        for (int j = 0; j < p; ++j) x[j] = get(state, m->dtype, ch * p + j);
        lr_hs_counters cnt = {0, 0, 0, 0};
        for (int64_t i = 0; i < o->iters; ++i) {
            for (int64_t t = 0; t < o->thin; ++t)
                cnt.skipped += (uint32_t)hs_sweep(m, bvec, &pr, o->seed, (uint64_t)(o->chain_offset + ch), (uint64_t)(o->iter_offset + i * o->thin + t), x, h, psi, om, &cnt);
            if (out)
                for (int j = 0; j < p; ++j) put(out, m->dtype, (i * C + ch) * p + j, x[j]);
            if (scale_out) {
                double *s = scale_out + (i * C + ch) * (p + 1);
                for (int j = 0; j < p; ++j) s[j] = pr.shrink[j] ? hs_sane(h[j]) : 1.0;
                s[p] = hs_sane(h[2 * p]);
            }
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
        h[2 * p] = hs_sane(h[2 * p]); /* (tau^2 and xi leave a launch as the sweep read them) */
        h[2 * p + 1] = hs_sane(h[2 * p + 1]);
        if (counters) {
            counters[ch].proposals += cnt.proposals;
            counters[ch].series_terms += cnt.series_terms;
            counters[ch].skipped += cnt.skipped;
            counters[ch].clamped += cnt.clamped;
        }
    }
    free(psi);
    return LR_OK;
}

LR_API int lr_hs_hyper(lr_model *m, const lr_hs_prior *prior, const void *state, const double *hyper_in, const lr_run_opts *o, double *hyper_out, lr_hs_counters *counters) {
    hs_prior pr;
    int rc = hs_check("lr_hs_hyper", m, prior, o, hyper_in, "hyper_in", &pr);
    if (rc) return rc;
    if (!o) return fail(LR_ERR_INVALID, "opts is NULL");
    if (!hyper_out) return fail(LR_ERR_INVALID, "hyper_out is NULL");
    lr_run_opts one = *o;
    one.iters = 1;
    one.thin = 1;
    one.stats = NULL;
    if ((rc = pg_check(m, &one))) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    const int p = m->p;
    for (int64_t ch = 0; ch < one.n_chains; ++ch) {
        double x[PG_MAXP];
        for (int j = 0; j < p; ++j) x[j] = get(state, m->dtype, ch * p + j);
        const uint32_t n = hs_hyper_step(p, &pr, one.seed, (uint64_t)(one.chain_offset + ch), (uint64_t)one.iter_offset, x, hyper_in + ch * (2 * p + 2), hyper_out + ch * (2 * p + 2));
        if (counters) counters[ch].clamped += n;
    }
    return LR_OK;
}
