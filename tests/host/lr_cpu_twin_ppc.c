/*
 * lr_cpu_twin_ppc.c -- the CPU TEST DOUBLE of include/logreg_hip_ppc.h: the whole ABI of lr_cpu_twin.c plus the lr_ppc_* entry points, in
 * float64 on the oracle's Philox stream.  TEST INFRASTRUCTURE ONLY (tests/twin_ppc.py builds and injects it).
 *
 * It follows the text of include/logreg_hip_ppc.h line by line: the pair quantities from one exponential and one log1p, the replicate
 * from word s & 3 of the block (q lo, q hi, i, LR_PPC_TAG), the per-draw counts and deviances, the tables.  Sums over rows run in index
 * order and the moments by Welford's update draw by draw (the device's run over its fixed trees): the integer tables of a float64 model
 * then equal the device's wherever no u lies within rounding of pi.
 */
#include "lr_cpu_twin.c"

#include "../../include/logreg_hip_ppc.h"

struct lr_ppc {
    lr_model *m;
    int p, G, labels;
    int64_t r, n, bad;
    uint64_t seed;
    double *X, *y; /* [r][p], [r] (own copies) */
    int32_t *grp;
    int64_t n_g[LR_PPC_MAX_GROUPS], t_obs[LR_PPC_MAX_GROUPS], off[LR_PPC_MAX_GROUPS];
    uint64_t *hist, *ones, dev_ge;
    double nf, mom[4];
};

LR_API void lr_ppc_destroy(lr_ppc *a) {
    if (!a) return;
    free(a->X);
    free(a->y);
    free(a->grp);
    free(a->hist);
    free(a->ones);
    free(a);
}

LR_API int lr_ppc_reset(lr_ppc *a) {
    if (!a) return fail(LR_ERR_INVALID, "lr_ppc_reset: accumulator is NULL");
    memset(a->hist, 0, sizeof(uint64_t) * (size_t)(a->r + a->G));
    memset(a->ones, 0, sizeof(uint64_t) * (size_t)a->r);
    memset(a->mom, 0, sizeof(a->mom));
    a->dev_ge = 0;
    a->n = a->bad = 0;
    a->nf = 0;
    return LR_OK;
}

LR_API int lr_ppc_create(lr_model *m, const double *X_new, const double *y_new, int64_t r, const int32_t *groups, int32_t G, uint64_t seed, lr_ppc **out) {
    if (!m || !out) return fail(LR_ERR_INVALID, "lr_ppc_create: model / out is NULL");
    if (r <= 0) return fail(LR_ERR_INVALID, "lr_ppc_create: r must be positive (got %lld)", (long long)r);
    if (G < 1 || G > LR_PPC_MAX_GROUPS) return fail(LR_ERR_INVALID, "lr_ppc_create: G must be 1 .. %d (got %d)", LR_PPC_MAX_GROUPS, G);
    if (!groups && G != 1) return fail(LR_ERR_INVALID, "lr_ppc_create: groups = NULL means one group, G = %d", G);
    if (!X_new && y_new) return fail(LR_ERR_INVALID, "lr_ppc_create: y_new without X_new (X_new = NULL means the model's own design AND labels)");
    if (!X_new && r != m->n) return fail(LR_ERR_INVALID, "lr_ppc_create: X_new = NULL means the model's own %lld rows, r = %lld", (long long)m->n, (long long)r);
    const int p = m->p;
    for (int64_t i = 0; i < r; ++i) {
        if (y_new && y_new[i] != 0.0 && y_new[i] != 1.0) return fail(LR_ERR_INVALID, "lr_ppc_create: y_new[%lld]=%g is not 0/1", (long long)i, y_new[i]);
        if (groups && (groups[i] < 0 || groups[i] >= G)) return fail(LR_ERR_INVALID, "lr_ppc_create: groups[%lld]=%d is outside [0, %d)", (long long)i, groups[i], G);
        if (X_new)
            for (int j = 0; j < p; ++j)
                if (!isfinite(X_new[i * p + j])) return fail(LR_ERR_INVALID, "lr_ppc_create: X_new[%lld,%d] is not finite", (long long)i, j);
    }
    lr_ppc *a = (lr_ppc *)calloc(1, sizeof(lr_ppc));
    if (!a) return fail(LR_ERR_NOMEM, "lr_ppc_create: handle");
    a->m = m;
    a->p = p;
    a->G = G;
    a->r = r;
    a->seed = seed;
    a->labels = !X_new || y_new;
    a->X = (double *)malloc(sizeof(double) * (size_t)(r * p));
    a->y = (double *)calloc((size_t)r, sizeof(double));
    a->grp = (int32_t *)calloc((size_t)r, sizeof(int32_t));
    a->hist = (uint64_t *)calloc((size_t)(r + G), sizeof(uint64_t));
    a->ones = (uint64_t *)calloc((size_t)r, sizeof(uint64_t));
    if (!a->X || !a->y || !a->grp || !a->hist || !a->ones) {
        lr_ppc_destroy(a);
        return fail(LR_ERR_NOMEM, "lr_ppc_create: tables");
    }
    for (int64_t i = 0; i < r; ++i) {
        for (int j = 0; j < p; ++j) {
            const double v = X_new ? X_new[i * p + j] : m->X[i * p + j];
            a->X[i * p + j] = m->dtype == LR_F32 ? (double)(float)v : v;
        }
        a->y[i] = X_new ? (y_new ? y_new[i] : 1.0) : m->y[i];
        a->grp[i] = groups ? groups[i] : 0;
        a->n_g[a->grp[i]] += 1;
        if (a->labels && a->y[i] > 0.5) a->t_obs[a->grp[i]] += 1;
    }
    for (int g = 0; g < G; ++g) {
        if (!a->labels) a->t_obs[g] = -1;
        a->off[g] = g ? a->off[g - 1] + a->n_g[g - 1] + 1 : 0;
    }
    *out = a;
    return LR_OK;
}

/* draw `theta` of index s -> counts [G], dev [2], bits [words] (may be NULL); returns 0 for a non-finite draw (zeros and NaN) */
static int ppc_draw(const lr_ppc *a, const double *theta, uint64_t s, int32_t *counts, double *dev, uint32_t *bits) {
    const int p = a->p;
    const int64_t words = (a->r + 31) / 32;
    int fin = 1;
    for (int j = 0; j < p; ++j) fin = fin && isfinite(theta[j]);
    for (int g = 0; g < a->G; ++g) counts[g] = 0;
    if (bits) memset(bits, 0, sizeof(uint32_t) * (size_t)words);
    dev[0] = dev[1] = NAN;
    if (!fin) return 0;
    double so = 0.0, sr = 0.0;
    const uint64_t q = s >> 2;
    for (int64_t i = 0; i < a->r; ++i) {
        double eta = 0.0;
        for (int j = 0; j < p; ++j) eta = fma(a->X[i * p + j], theta[j], eta);
        const double e = exp(-fabs(eta)), rc = 1.0 / (1.0 + e), lp = log1p(e);
        const double pi = eta >= 0 ? rc : e * rc;
        const double l1 = (eta < 0 ? eta : 0.0) - lp, l0 = (eta > 0 ? -eta : 0.0) - lp;
        uint32_t w[4];
        stream_block(a->seed, q & 0xFFFFFFFFu, (q >> 32) | ((uint64_t)i << 32), LR_PPC_TAG, w);
        const uint32_t hi = w[s & 3] >> 8;
        const double u = a->m->dtype == LR_F32 ? (double)(((float)hi + 0.5f) * (1.0f / 16777216.0f)) : ((double)hi + 0.5) * (1.0 / 16777216.0);
        const int rep = u < pi;
        if (rep) {
            counts[a->grp[i]] += 1;
            if (bits) bits[i >> 5] |= 1u << (i & 31);
        }
        so += a->y[i] > 0.5 ? l1 : l0;
        sr += rep ? l1 : l0;
    }
    dev[0] = a->labels ? -2.0 * so : NAN;
    dev[1] = -2.0 * sr;
    return 1;
}

LR_API int lr_ppc_accumulate(lr_ppc *a, const void *draws, int64_t S, int32_t on_device, void *stream) {
    (void)on_device;
    (void)stream;
    if (!a || !draws) return fail(LR_ERR_INVALID, "lr_ppc_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_ppc_accumulate: S must be positive (got %lld)", (long long)S);
    const int64_t words = (a->r + 31) / 32;
    uint32_t *bits = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)words);
    if (!bits) return fail(LR_ERR_NOMEM, "lr_ppc_accumulate: bits");
    double theta[128], dev[2];
    int32_t counts[LR_PPC_MAX_GROUPS];
    for (int64_t k = 0; k < S; ++k, ++a->n) {
        for (int j = 0; j < a->p; ++j) theta[j] = get(draws, a->m->dtype, k * a->p + j);
        if (!ppc_draw(a, theta, (uint64_t)a->n, counts, dev, bits)) {
            a->bad += 1;
            continue;
        }
        for (int g = 0; g < a->G; ++g) a->hist[a->off[g] + counts[g]] += 1;
        for (int64_t i = 0; i < a->r; ++i) a->ones[i] += (bits[i >> 5] >> (i & 31)) & 1u;
        if (dev[1] >= dev[0]) a->dev_ge += 1;
        a->nf += 1;
        for (int k2 = 0; k2 < 2; ++k2) {
            const double d = dev[k2] - a->mom[2 * k2];
            a->mom[2 * k2] += d / a->nf;
            a->mom[2 * k2 + 1] += d * (dev[k2] - a->mom[2 * k2]);
        }
    }
    free(bits);
    return LR_OK;
}

LR_API int lr_ppc_terms(lr_ppc *a, const void *draws, int64_t S, int64_t first_index, int32_t on_device, void *stream, int32_t *counts_out, double *dev_out,
                        uint32_t *yrep_out) {
    (void)on_device;
    (void)stream;
    if (!a || !draws || !counts_out || !dev_out) return fail(LR_ERR_INVALID, "lr_ppc_terms: accumulator / draws / counts_out / dev_out is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_ppc_terms: S must be positive (got %lld)", (long long)S);
    if (first_index < 0) return fail(LR_ERR_INVALID, "lr_ppc_terms: first_index must be >= 0 (got %lld)", (long long)first_index);
    const int64_t words = (a->r + 31) / 32;
    double theta[128];
    for (int64_t k = 0; k < S; ++k) {
        for (int j = 0; j < a->p; ++j) theta[j] = get(draws, a->m->dtype, k * a->p + j);
        ppc_draw(a, theta, (uint64_t)(first_index + k), counts_out + k * a->G, dev_out + 2 * k, yrep_out ? yrep_out + k * words : NULL);
    }
    return LR_OK;
}

LR_API int lr_ppc_result(lr_ppc *a, uint64_t *hist, uint64_t *row_ones, uint64_t *counts, double *moments, int64_t *t_obs, int64_t *n_g, int64_t *n_draws) {
    if (!a) return fail(LR_ERR_INVALID, "lr_ppc_result: accumulator is NULL");
    if (hist) memcpy(hist, a->hist, sizeof(uint64_t) * (size_t)(a->r + a->G));
    if (row_ones) memcpy(row_ones, a->ones, sizeof(uint64_t) * (size_t)a->r);
    if (counts) {
        counts[0] = a->dev_ge;
        counts[1] = (uint64_t)a->bad;
    }
    if (moments)
        for (int k = 0; k < LR_PPC_MOMENTS; ++k) moments[k] = a->nf > 0 && (a->labels || k >= 2) ? a->mom[k] : NAN;
    if (t_obs) memcpy(t_obs, a->t_obs, sizeof(int64_t) * (size_t)a->G);
    if (n_g) memcpy(n_g, a->n_g, sizeof(int64_t) * (size_t)a->G);
    if (n_draws) *n_draws = a->n;
    return LR_OK;
}
