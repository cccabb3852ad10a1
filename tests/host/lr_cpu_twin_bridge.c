/*
 * lr_cpu_twin_bridge.c -- the CPU TEST DOUBLE of include/logreg_hip_bridge.h: the whole ABI of lr_cpu_twin.c plus the lr_bridge_* entry
 * points, in float64 on the oracle's Philox stream.  TEST INFRASTRUCTURE ONLY (tests/twin_bridge.py builds and injects it).
 *
 * It follows the text of include/logreg_hip_bridge.h step by step: the factor and its inverse by the same substitutions, the term of a
 * draw as it is stored in the model's dtype, the proposal draws from (seed, j), the iteration shifted by its largest terms, the error from
 * shifted sums.  Sums over rows and over terms run in index order here (the device's run over its fixed trees): a float64 model then
 * differs from the device by the order of the sums and the last bits of log / exp alone.
 */
#include "lr_cpu_twin.c"

#include "../../include/logreg_hip_bridge.h"

struct lr_bridge {
    lr_model *m;
    int p;
    int64_t cap, N1, N2;
    uint64_t seed;
    double cg;
    double *mu, *L, *W; /* [p], packed lower triangles [p (p + 1) / 2] */
    double *l1, *l2;
};

static int br_factor(int p, const double *mu, const double *cov, double *Lp, double *Wp, double *cg) {
    for (int i = 0; i < p; ++i) {
        if (!isfinite(mu[i])) return fail(LR_ERR_INVALID, "lr_bridge_create: mu[%d] is not finite", i);
        for (int j = 0; j <= i; ++j)
            if (!isfinite(cov[i * p + j])) return fail(LR_ERR_INVALID, "lr_bridge_create: cov[%d][%d] is not finite", i, j);
    }
    double *L = (double *)calloc((size_t)p * p, sizeof(double)), *W = (double *)calloc((size_t)p * p, sizeof(double));
    if (!L || !W) {
        free(L);
        free(W);
        return fail(LR_ERR_NOMEM, "lr_bridge_create: factor");
    }
    double logdet = 0.0;
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            double t = cov[i * p + j];
            for (int k = 0; k < j; ++k) t = t - L[i * p + k] * L[j * p + k];
            if (i == j) {
                if (!(t > 0) || !isfinite(t)) {
                    free(L);
                    free(W);
                    return fail(LR_ERR_INVALID, "lr_bridge_create: cov is not positive definite: pivot %d is %g", i, t);
                }
                L[i * p + i] = sqrt(t);
                logdet = logdet + log(L[i * p + i]);
            } else {
                L[i * p + j] = t / L[j * p + j];
            }
        }
    for (int c = 0; c < p; ++c)
        for (int i = c; i < p; ++i) {
            double t = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) t = t - L[i * p + k] * W[k * p + c];
            W[i * p + c] = t / L[i * p + i];
        }
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            Lp[i * (i + 1) / 2 + j] = L[i * p + j];
            Wp[i * (i + 1) / 2 + j] = W[i * p + j];
        }
    free(L);
    free(W);
    *cg = -logdet - 0.5 * p * 1.8378770664093453;
    return LR_OK;
}

/* l = lpost - log g of a draw theta [p] (already as the model's dtype stores it) */
static double br_term(const lr_bridge *a, const double *theta) {
    const lr_model *m = a->m;
    const int p = a->p;
    double ll = 0.0, pr = 0.0, q = 0.0, lpc = 0.0;
    for (int64_t i = 0; i < m->n; ++i) {
        double eta = 0.0;
        for (int j = 0; j < p; ++j) eta = fma(m->X[i * p + j], theta[j], eta);
        const double t = (2.0 * m->y[i] - 1.0) * eta;
        ll += (t < 0 ? t : 0.0) - log1p(exp(-fabs(t)));
    }
    for (int j = 0; j < p; ++j) {
        const double iv = 1.0 / (m->sd[j] * m->sd[j]);
        pr = fma(iv * theta[j], theta[j], pr);
        lpc += -log(m->sd[j]) - 0.91893853320467274178;
    }
    const double *Wrow = a->W;
    for (int i = 0; i < p; ++i) {
        double yv = 0.0;
        for (int j = 0; j <= i; ++j) yv = fma(Wrow[j], theta[j] - a->mu[j], yv);
        q = fma(yv, yv, q);
        Wrow += i + 1;
    }
    return (ll + fma(-0.5, pr, lpc)) - fma(-0.5, q, a->cg);
}

/* proposal draw j -> theta [p], rounded to the model's dtype */
static void br_propose(const lr_bridge *a, uint64_t j, double *theta) {
    const int p = a->p;
    double z[128 + 4];
    const double two_pi = 6.283185307179586476925286766559;
    for (int b = 0; 4 * b < p; ++b) {
        uint32_t w[4];
        stream_block(a->seed, j & 0xFFFFFFFFu, j >> 32, LR_BRIDGE_TAG | (uint32_t)b, w);
        for (int h = 0; h < 2; ++h) {
            const double r = sqrt(-2.0 * log(u01(w[2 * h]))), th = two_pi * u01(w[2 * h + 1]);
            z[4 * b + 2 * h] = r * cos(th);
            z[4 * b + 2 * h + 1] = r * sin(th);
        }
    }
    const double *Lrow = a->L;
    for (int i = 0; i < p; ++i) {
        double t = a->mu[i];
        for (int c = 0; c <= i; ++c) t = fma(Lrow[c], z[c], t);
        theta[i] = a->m->dtype == LR_F32 ? (double)(float)t : t;
        Lrow += i + 1;
    }
}

static double br_lae(double x, double y) {
    const double m = x > y ? x : y;
    return m + log1p(exp(-fabs(x - y)));
}

static int br_check_solve(const char *who, double tol, int maxit) {
    if (!(tol >= 0.0)) return fail(LR_ERR_INVALID, "%s: tol must be >= 0 (got %g)", who, tol);
    if (maxit < 0) return fail(LR_ERR_INVALID, "%s: maxit must be >= 0 (got %d)", who, maxit);
    return LR_OK;
}

static void br_solve(const double *l1, int64_t N1, const double *l2, int64_t N2, double n_eff, double tol, int maxit, double *table) {
    const double n1 = (double)N1, n2 = (double)N2, neff = n_eff > 0 && isfinite(n_eff) ? n_eff : n1;
    const double s1 = neff / (neff + n2), s2 = n2 / (neff + n2), ls1 = log(s1), ls2 = log(s2);
    double mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY}, bad = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double *v = k ? l2 : l1;
        for (int64_t e = 0; e < (k ? N2 : N1); ++e) {
            if (!isfinite(v[e])) bad += 1.0;
            else {
                if (v[e] < mn[k]) mn[k] = v[e];
                if (v[e] > mx[k]) mx[k] = v[e];
            }
        }
    }
    for (int r = 0; r < LR_BRIDGE_ROWS; ++r) table[r] = NAN;
    table[2] = table[3] = 0.0;
    table[4] = n1;
    table[5] = n2;
    table[6] = neff;
    table[7] = bad;
    table[8] = mn[0] <= mx[0] ? mn[0] : NAN;
    table[9] = mn[0] <= mx[0] ? mx[0] : NAN;
    table[10] = mn[1] <= mx[1] ? mn[1] : NAN;
    table[11] = mn[1] <= mx[1] ? mx[1] : NAN;
    if (bad != 0.0) return;
    const double min1 = mn[0], max2 = mx[1];
    double sum = 0.0;
    for (int64_t e = 0; e < N2; ++e) sum += exp(l2[e] - max2);
    double lr = max2 + (log(sum) - log(n2));
    int it = 0, conv = 0;
    while (it < maxit && !conv) {
        const double c = ls2 + lr, top2 = max2 - br_lae(ls1 + max2, c), top1 = -br_lae(ls1 + min1, c);
        double sum2 = 0.0, sum1 = 0.0;
        for (int64_t e = 0; e < N2; ++e) sum2 += exp((l2[e] - br_lae(ls1 + l2[e], c)) - top2);
        for (int64_t e = 0; e < N1; ++e) sum1 += exp(-br_lae(ls1 + l1[e], c) - top1);
        const double tops = max2 + (br_lae(ls1 + min1, c) - br_lae(ls1 + max2, c));
        const double next = tops + ((log(sum2) - log(n2)) - (log(sum1) - log(n1)));
        ++it;
        conv = fabs(next - lr) <= tol * (fabs(next) > 1.0 ? fabs(next) : 1.0);
        lr = next;
    }
    const double c2 = 1.0 / fma(s2, exp(lr - max2), s1), c1 = 1.0 / fma(s1, exp(min1 - lr), s2);
    double d2 = 0.0, q2 = 0.0, d1 = 0.0, q1 = 0.0;
    for (int64_t e = 0; e < N2; ++e) {
        const double d = 1.0 / fma(s2, exp(lr - l2[e]), s1) - c2;
        d2 += d;
        q2 = fma(d, d, q2);
    }
    for (int64_t e = 0; e < N1; ++e) {
        const double d = 1.0 / fma(s1, exp(l1[e] - lr), s2) - c1;
        d1 += d;
        q1 = fma(d, d, q1);
    }
    const double m2 = c2 + d2 / n2, m1 = c1 + d1 / n1;
    const double v2 = n2 > 1.0 ? fma(-d2 / n2, d2, q2) / (n2 - 1.0) : 0.0, v1 = n1 > 1.0 ? fma(-d1 / n1, d1, q1) / (n1 - 1.0) : 0.0;
    table[0] = lr;
    table[1] = sqrt(v2 / (m2 * m2 * n2) + v1 / (m1 * m1 * neff));
    table[2] = (double)it;
    table[3] = (double)conv;
}

LR_API void lr_bridge_destroy(lr_bridge *a) {
    if (!a) return;
    free(a->mu);
    free(a->L);
    free(a->W);
    free(a->l1);
    free(a->l2);
    free(a);
}

LR_API int lr_bridge_create(lr_model *m, const double *mu, const double *cov, int64_t max_draws, int64_t n_proposal, uint64_t seed, lr_bridge **out) {
    if (!m || !mu || !cov || !out) return fail(LR_ERR_INVALID, "lr_bridge_create: model / mu / cov / out is NULL");
    if (max_draws <= 0 || n_proposal <= 0)
        return fail(LR_ERR_INVALID, "lr_bridge_create: max_draws and n_proposal must be positive (got %lld, %lld)", (long long)max_draws, (long long)n_proposal);
    if (max_draws > LR_BRIDGE_MAX_DRAWS || n_proposal > LR_BRIDGE_MAX_DRAWS) return fail(LR_ERR_UNSUPPORTED, "lr_bridge_create: beyond LR_BRIDGE_MAX_DRAWS");
    lr_bridge *a = (lr_bridge *)calloc(1, sizeof(lr_bridge));
    if (!a) return fail(LR_ERR_NOMEM, "lr_bridge_create: handle");
    const int p = m->p;
    const size_t tri = (size_t)p * (p + 1) / 2;
    a->m = m;
    a->p = p;
    a->cap = max_draws;
    a->N2 = n_proposal;
    a->seed = seed;
    a->mu = (double *)malloc(sizeof(double) * (size_t)p);
    a->L = (double *)malloc(sizeof(double) * tri);
    a->W = (double *)malloc(sizeof(double) * tri);
    a->l1 = (double *)malloc(sizeof(double) * (size_t)max_draws);
    a->l2 = (double *)malloc(sizeof(double) * (size_t)n_proposal);
    if (!a->mu || !a->L || !a->W || !a->l1 || !a->l2) {
        lr_bridge_destroy(a);
        return fail(LR_ERR_NOMEM, "lr_bridge_create: terms");
    }
    const int rc = br_factor(p, mu, cov, a->L, a->W, &a->cg);
    if (rc) {
        lr_bridge_destroy(a);
        return rc;
    }
    memcpy(a->mu, mu, sizeof(double) * (size_t)p);
    double theta[128];
    for (int64_t j = 0; j < n_proposal; ++j) {
        br_propose(a, (uint64_t)j, theta);
        a->l2[j] = br_term(a, theta);
    }
    *out = a;
    return LR_OK;
}

LR_API int lr_bridge_accumulate(lr_bridge *a, const void *draws, int64_t S, int32_t on_device, void *stream) {
    (void)on_device;
    (void)stream;
    if (!a || !draws) return fail(LR_ERR_INVALID, "lr_bridge_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_bridge_accumulate: S must be positive (got %lld)", (long long)S);
    if (S > a->cap - a->N1)
        return fail(LR_ERR_INVALID, "lr_bridge_accumulate: %lld draws held + %lld more exceed max_draws = %lld", (long long)a->N1, (long long)S, (long long)a->cap);
    double theta[128];
    for (int64_t s = 0; s < S; ++s) {
        for (int j = 0; j < a->p; ++j) theta[j] = get(draws, a->m->dtype, s * a->p + j);
        a->l1[a->N1 + s] = br_term(a, theta);
    }
    a->N1 += S;
    return LR_OK;
}

LR_API int lr_bridge_terms(lr_bridge *a, double *l1, double *l2, int64_t *n1, int64_t *n2) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_terms: accumulator is NULL");
    if (n1) *n1 = a->N1;
    if (n2) *n2 = a->N2;
    if (l1) memcpy(l1, a->l1, sizeof(double) * (size_t)a->N1);
    if (l2) memcpy(l2, a->l2, sizeof(double) * (size_t)a->N2);
    return LR_OK;
}

LR_API int lr_bridge_proposal(lr_bridge *a, void *host_out, int64_t *n2) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_proposal: accumulator is NULL");
    if (n2) *n2 = a->N2;
    if (!host_out) return LR_OK;
    double theta[128];
    for (int64_t j = 0; j < a->N2; ++j) {
        br_propose(a, (uint64_t)j, theta);
        for (int i = 0; i < a->p; ++i) put(host_out, a->m->dtype, j * a->p + i, theta[i]);
    }
    return LR_OK;
}

LR_API int lr_bridge_result(lr_bridge *a, double n_eff, double tol, int32_t maxit, double *table) {
    if (!a || !table) return fail(LR_ERR_INVALID, "lr_bridge_result: accumulator / table is NULL");
    const int rc = br_check_solve("lr_bridge_result", tol, maxit);
    if (rc) return rc;
    if (a->N1 == 0) {
        for (int r = 0; r < LR_BRIDGE_ROWS; ++r) table[r] = NAN;
        table[2] = table[3] = table[4] = 0.0;
        table[5] = (double)a->N2;
        return LR_OK;
    }
    br_solve(a->l1, a->N1, a->l2, a->N2, n_eff, tol, maxit, table);
    return LR_OK;
}

LR_API int lr_bridge_reset(lr_bridge *a) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_reset: accumulator is NULL");
    a->N1 = 0;
    return LR_OK;
}

LR_API int lr_bridge_solve(int device, const double *l1, int64_t N1, const double *l2, int64_t N2, double n_eff, double tol, int32_t maxit,
                           int32_t on_device, double *table, void *stream) {
    (void)on_device;
    (void)stream;
    if (!l1 || !l2 || !table) return fail(LR_ERR_INVALID, "lr_bridge_solve: l1 / l2 / table is NULL");
    if (N1 <= 0 || N2 <= 0) return fail(LR_ERR_INVALID, "lr_bridge_solve: N1 and N2 must be positive (got %lld, %lld)", (long long)N1, (long long)N2);
    const int rc = br_check_solve("lr_bridge_solve", tol, maxit);
    if (rc) return rc;
    if (device != 0) return fail(LR_ERR_HIP, "lr_bridge_solve: device %d not available (1 visible)", device);
    br_solve(l1, N1, l2, N2, n_eff, tol, maxit, table);
    return LR_OK;
}
