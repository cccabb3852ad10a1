/*
 * lr_cpu_twin_pg.c -- the CPU TEST DOUBLE of include/logreg_hip_pg.h: the whole ABI of lr_cpu_twin.c plus lr_run_pg and lr_pg_omega, in
 * float64 on the oracle's Philox stream.  TEST INFRASTRUCTURE ONLY (tests/twin_pg.py builds and injects it).
 *
 * It follows the text of include/logreg_hip_pg.h decision by decision and word by word, and sums as the kernel (logreg_amd/csrc/lr_pg.h)
 * does: A in row order with one fma per entry, the column-oriented forward solve with one fma per entry, the backward solve's sums in the
 * order of a 16-lane butterfly.  A float64 model then differs from the device only by the last bits of log / exp / erfc / cos.
 */
/* the base double's planner knows kinds 0..3: its entry points are renamed and wrapped below */
#define lr_plan_run twin_base_plan_run
#define lr_plan_run_info twin_base_plan_run_info
#include "lr_cpu_twin.c"
#undef lr_plan_run
#undef lr_plan_run_info

#include "../../include/logreg_hip_pg.h"

LR_API int lr_plan_run(const lr_model *m, int32_t kind, const lr_run_opts *o, int32_t *mode_out, int32_t *group_out, int32_t *rows_out) {
    int rc = check_opts(m, o, 0);
    if (rc) return rc;
    if ((kind < LR_KIND_RWMH || kind > LR_KIND_UL) && kind != LR_KIND_PG) return fail(LR_ERR_INVALID, "unknown kernel family %d", kind);
    if (kind == LR_KIND_PG && m->p > 32) return fail(LR_ERR_UNSUPPORTED, "PG: p = %d > 32", m->p);
    if (kind == LR_KIND_PG && m->n >= LR_PG_MAX_ROWS) return fail(LR_ERR_UNSUPPORTED, "PG: n = %lld >= %d", (long long)m->n, LR_PG_MAX_ROWS);
    return lr_plan(m, o->plan_chains > 0 ? o->plan_chains : o->n_chains, o->group, o->mode, mode_out, group_out, rows_out);
}
LR_API int lr_plan_run_info(const lr_model *m, int32_t kind, const lr_run_opts *opts, lr_plan_info *out) {
    if (!out) return fail(LR_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof *out);
    return lr_plan_run(m, kind, opts, &out->mode, &out->group, &out->rows);
}

#define PG_MAXP 32
#define PG_PI 3.14159265358979323846
#define PG_T 0.64

typedef struct {
    uint64_t seed, chain, iter;
    uint32_t row, cursor, w[4];
} pg_words;
static uint32_t pg_next(pg_words *s) {
    if ((s->cursor & 3u) == 0) stream_block(s->seed, s->chain, s->iter, LR_PG_TAG | ((s->cursor >> 2) << 16) | s->row, s->w);
    return s->w[s->cursor++ & 3u];
}
static double pg_coef(int n, double x, int small) {
    const double h = (double)n + 0.5;
    if (small) {
        const double v = 2.0 / (PG_PI * x);
        return PG_PI * h * (v * sqrt(v)) * exp(-2.0 * h * h / x);
    }
    return PG_PI * h * exp(-(h * h) * (PG_PI * PG_PI * 0.5) * x);
}
/* omega ~ PG(1, |psi|): include/logreg_hip_pg.h "The draw" */
static double pg_draw(double psi, uint64_t seed, uint64_t chain, uint64_t iter, uint32_t row, uint64_t *nprop, uint64_t *nterm) {
    const double t = PG_T, z = 0.5 * fabs(psi), K = PG_PI * PG_PI * 0.125 + 0.5 * z * z;
    double r = 0.0;
    if (z < 10.0) {
        const double kt = K * t;
        const double pb = 0.5 * erfc(-((t * z - 1.0) / 0.8) * 0.70710678118654752440);
        const double pa = 0.5 * erfc(((t * z + 1.0) / 0.8) * 0.70710678118654752440);
        r = 1.0 / (1.0 + (4.0 / PG_PI) * K * (exp(kt - z) * pb + exp(kt + z) * pa));
    }
    const int pair = z < 1.0 / PG_T;
    const double mu = 1.0 / z;
    pg_words ws = {seed, chain, iter, row, 0, {0, 0, 0, 0}};
    double X = t;
    for (int round = 0; round < LR_PG_MAX_ROUNDS; ++round) {
        ++*nprop;
        const double U = u01(pg_next(&ws));
        if (U < r) {
            const double E = -log(u01(pg_next(&ws)));
            X = t + E / K;
        } else {
            for (int trial = 0; trial < LR_PG_MAX_TRIALS; ++trial) {
                const double ua = u01(pg_next(&ws)), ub = u01(pg_next(&ws)), uc = u01(pg_next(&ws));
                int ok;
                if (pair) {
                    const double E1 = -log(ua), E2 = -log(ub), d = 1.0 + t * E1;
                    X = t / (d * d);
                    ok = (E1 * E1 <= 2.0 * E2 / t) && (uc <= exp(-0.5 * z * z * X));
                } else {
                    const double N = sqrt(-2.0 * log(ua)) * cos(2.0 * PG_PI * ub);
                    const double w = 0.5 * mu * (N * N), s = 1.0 + w + sqrt(w * (w + 2.0));
                    X = mu / s;
                    if (uc > mu / (mu + X)) X = mu * s;
                    ok = X <= t;
                }
                if (ok) break;
                if (trial == LR_PG_MAX_TRIALS - 1) X = X > t ? t : X;
            }
        }
        const int small = X <= t;
        const double V = u01(pg_next(&ws));
        double S = pg_coef(0, X, small);
        const double Y = V * S;
        int accept = 1;
        for (int n = 1; n <= LR_PG_MAX_TERMS; ++n) {
            ++*nterm;
            const double an = pg_coef(n, X, small);
            if (n & 1) {
                S -= an;
                if (Y <= S) break;
            } else {
                S += an;
                if (Y > S) {
                    accept = 0;
                    break;
                }
            }
        }
        if (accept) break;
    }
    return 0.25 * X;
}

/* the sum of the 16 lanes' values in the order of group_sum<16> (lr_device.h): mirror, half mirror, two quad permutes */
static double pg_sum16(const double *v) {
    double a[16], b[16];
    for (int i = 0; i < 16; ++i) a[i] = v[i] + v[15 - i];
    for (int i = 0; i < 16; ++i) b[i] = a[i] + a[(i & 8) | (7 - (i & 7))];
    for (int i = 0; i < 16; ++i) a[i] = b[i] + b[i ^ 2];
    return a[0] + a[1];
}

static double pg_xs(const lr_model *m, int64_t i, int j) { return (2.0 * m->y[i] - 1.0) * m->X[i * m->p + j]; }

/* psi of every row at beta; returns 0 if one is not finite */
static int pg_psi(const lr_model *m, const double *beta, double *psi) {
    int fin = 1;
    for (int64_t i = 0; i < m->n; ++i) {
        double s = 0.0;
        for (int j = 0; j < m->p; ++j) s = fma(pg_xs(m, i, j), beta[j], s);
        psi[i] = s;
        fin = fin && isfinite(s);
    }
    return fin;
}

/* one sweep of one chain; beta in/out.  Returns 1 if the chain stayed in place. */
static int pg_sweep(const lr_model *m, const double *bvec, uint64_t seed, uint64_t chain, uint64_t iter, double *beta, double *psi, double *om,
                    lr_pg_counters *cnt) {
    const int p = m->p;
    const int fin = pg_psi(m, beta, psi);
    if (!fin) return 1;
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
    for (int j = 0; j < p; ++j) {
        A[j][j] += 1.0 / (m->sd[j] * m->sd[j]);
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
    for (int j = 0; j < p; ++j) beta[j] = d[j] * x[j];
    cnt->proposals += nprop;
    cnt->series_terms += nterm;
    return 0;
}

static int pg_check(const lr_model *m, const lr_run_opts *o) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    int rc = check_opts(m, o, 1);
    if (rc) return rc;
    if (m->p > 32) return fail(LR_ERR_UNSUPPORTED, "PG: p = %d > 32", m->p);
    if (m->n >= LR_PG_MAX_ROWS) return fail(LR_ERR_UNSUPPORTED, "PG: n = %lld >= %d", (long long)m->n, LR_PG_MAX_ROWS);
    return LR_OK;
}
static void pg_bvec(const lr_model *m, double *b) {
    for (int j = 0; j < m->p; ++j) b[j] = 0.0;
    for (int64_t i = 0; i < m->n; ++i)
        for (int j = 0; j < m->p; ++j) b[j] += pg_xs(m, i, j);
    for (int j = 0; j < m->p; ++j) b[j] *= 0.5;
}

LR_API int lr_run_pg(lr_model *m, void *state, const lr_run_opts *o, void *out, lr_pg_counters *counters) {
    int rc = pg_check(m, o);
    if (rc) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    const int p = m->p;
    const int64_t C = o->n_chains;
    double bvec[PG_MAXP];
    pg_bvec(m, bvec);
    double *psi = (double *)malloc(sizeof(double) * (size_t)m->n * 2), *om = psi + m->n;
    if (!psi) return fail(LR_ERR_NOMEM, "run scratch");
    for (int64_t ch = 0; ch < C; ++ch) {
        double x[PG_MAXP];
        for (int j = 0; j < p; ++j) x[j] = get(state, m->dtype, ch * p + j);
        lr_pg_counters cnt = {0, 0, 0, 0};
        for (int64_t i = 0; i < o->iters; ++i) {
            for (int64_t t = 0; t < o->thin; ++t) {
                cnt.skipped += (uint32_t)pg_sweep(m, bvec, o->seed, (uint64_t)(o->chain_offset + ch), (uint64_t)(o->iter_offset + i * o->thin + t), x, psi, om, &cnt);
                if (m->dtype == LR_F32) /* the state as the device holds it between sweeps */
                    for (int j = 0; j < p; ++j) x[j] = (double)(float)x[j];
            }
            if (out)
                for (int j = 0; j < p; ++j) put(out, m->dtype, (i * C + ch) * p + j, x[j]);
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
            counters[ch].proposals += cnt.proposals;
            counters[ch].series_terms += cnt.series_terms;
            counters[ch].skipped += cnt.skipped;
        }
    }
    free(psi);
    return LR_OK;
}

LR_API int lr_pg_omega(lr_model *m, const void *state, const lr_run_opts *o, void *omega_out) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!o) return fail(LR_ERR_INVALID, "opts is NULL");
    if (!omega_out) return fail(LR_ERR_INVALID, "omega_out is NULL");
    lr_run_opts one = *o;
    one.iters = 1;
    one.thin = 1;
    one.stats = NULL;
    int rc = pg_check(m, &one);
    if (rc) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    const int p = m->p;
    double *psi = (double *)malloc(sizeof(double) * (size_t)m->n);
    if (!psi) return fail(LR_ERR_NOMEM, "scratch");
    for (int64_t ch = 0; ch < one.n_chains; ++ch) {
        double x[PG_MAXP];
        uint64_t np_ = 0, nt_ = 0;
        for (int j = 0; j < p; ++j) x[j] = get(state, m->dtype, ch * p + j);
        (void)pg_psi(m, x, psi);
        for (int64_t i = 0; i < m->n; ++i)
            put(omega_out, m->dtype, ch * m->n + i,
                isfinite(psi[i]) ? pg_draw(psi[i], one.seed, (uint64_t)(one.chain_offset + ch), (uint64_t)one.iter_offset, (uint32_t)i, &np_, &nt_) : NAN);
    }
    free(psi);
    return LR_OK;
}
