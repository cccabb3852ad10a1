/*
 * lr_cpu_twin_rank.c -- the CPU TEST DOUBLE of include/logreg_hip_rank.h: the whole ABI of lr_cpu_twin.c plus the lr_rank_* entry
 * points.  TEST INFRASTRUCTURE ONLY (tests/twin_rank.py builds and injects it).
 *
 * It follows the text of include/logreg_hip_rank.h step by step and shares the scalar arithmetic of the device
 * (logreg_amd/csrc/lr_rank_math.h: the key of a double, AS 241, the float64 finish of the tables).  The order comes from qsort on the keys;
 * sums over time and over chains run in index order here (the device's run over its fixed trees).
 */
#include "lr_cpu_twin.c"

#include "../../include/logreg_hip_rank.h"
#include "../../logreg_amd/csrc/lr_rank_math.h"

struct lr_rank {
    int dtype, p, K;
    int64_t C, max_steps, n;
    void *store;
};

static size_t rk_esize(const lr_rank *r) { return r->dtype == LR_F32 ? 4 : 8; }
static double rk_at(const lr_rank *r, int64_t i, int j) {
    return r->dtype == LR_F32 ? (double)((const float *)r->store)[i * r->p + j] : ((const double *)r->store)[i * r->p + j];
}
static int rk_cmp(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}
static int64_t rk_bound(const uint64_t *s, int64_t S, uint64_t key, int upper) {
    int64_t lo = 0, hi = S;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (upper ? s[mid] <= key : s[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

int lr_rank_create(int device, int32_t dtype, int64_t C, int32_t p, int64_t max_steps, int32_t max_lag, lr_rank **out) {
    (void)device;
    if (!out) return fail(LR_ERR_INVALID, "lr_rank_create: out is NULL");
    if (C <= 0 || p <= 0 || max_steps <= 0) return fail(LR_ERR_INVALID, "lr_rank_create: C, p and max_steps must be positive");
    if (max_lag < 1 || max_lag > LR_RANK_MAX_LAG || max_lag % 2 == 0) return fail(LR_ERR_INVALID, "lr_rank_create: max_lag must be odd and in 1..%d (got %d)", LR_RANK_MAX_LAG, max_lag);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_rank_create: dtype must be LR_F32 or LR_F64");
    if (C > LR_RANK_MAX_DRAWS || max_steps > LR_RANK_MAX_DRAWS / C) return fail(LR_ERR_UNSUPPORTED, "lr_rank_create: more than the cap of %lld draws per coordinate (LR_RANK_MAX_DRAWS)", (long long)LR_RANK_MAX_DRAWS);
    lr_rank *r = (lr_rank *)calloc(1, sizeof(lr_rank));
    if (!r) return fail(LR_ERR_NOMEM, "lr_rank_create");
    r->dtype = dtype, r->p = p, r->K = max_lag, r->C = C, r->max_steps = max_steps;
    r->store = malloc((size_t)max_steps * C * p * rk_esize(r));
    if (!r->store) {
        free(r);
        return fail(LR_ERR_NOMEM, "lr_rank_create: draws");
    }
    *out = r;
    return LR_OK;
}

int lr_rank_accumulate(lr_rank *r, const void *block, int64_t k, int32_t on_device, void *stream) {
    (void)on_device, (void)stream;
    if (!r || !block) return fail(LR_ERR_INVALID, "lr_rank_accumulate: accumulator / block is NULL");
    if (k <= 0) return fail(LR_ERR_INVALID, "lr_rank_accumulate: k must be positive");
    if (k > r->max_steps - r->n) return fail(LR_ERR_INVALID, "lr_rank_accumulate: %lld more steps after %lld exceed max_steps = %lld", (long long)k, (long long)r->n, (long long)r->max_steps);
    const size_t row = (size_t)r->C * r->p * rk_esize(r);
    memcpy((char *)r->store + (size_t)r->n * row, block, (size_t)k * row);
    r->n += k;
    return LR_OK;
}

/* keys of coordinate j (fold: of |x - med|) in time order into U, sorted into Ks */
static void rk_keys(const lr_rank *r, int j, int64_t S, int fold, double med, uint64_t *U, uint64_t *Ks) {
    for (int64_t i = 0; i < S; ++i) {
        const double x = rk_at(r, i, j);
        U[i] = Ks[i] = lr_rank_key(fold ? fabs(lr_rank_unkey(lr_rank_key(x)) - med) : x);
    }
    qsort(Ks, (size_t)S, sizeof(uint64_t), rk_cmp);
}

static void rk_rank(const uint64_t *U, const uint64_t *Ks, int64_t S, int64_t *r2) {
    for (int64_t i = 0; i < S; ++i) r2[i] = rk_bound(Ks, S, U[i], 0) + rk_bound(Ks, S, U[i], 1) + 1;
}

/* tab [2 + L + 1] of the series v [M][h] */
static void rk_table(const double *v, int64_t h, int64_t M, int L, double *tab, double *e) {
    double mean0 = 0.0;
    for (int l = 0; l < LR_RANK_TAB_HEAD + L + 1; ++l) tab[l] = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const double *vm = v + m * h;
        double s = 0.0;
        for (int64_t t = 0; t < h; ++t) s += vm[t] - vm[0];
        const double dbar = s / (double)h, mean = vm[0] + dbar;
        if (m == 0) mean0 = mean;
        for (int64_t t = 0; t < h; ++t) e[t] = (vm[t] - vm[0]) - dbar;
        tab[0] += mean - mean0;
        tab[1] += (mean - mean0) * (mean - mean0);
        for (int l = 0; l <= L; ++l) {
            double acc = 0.0;
            for (int64_t t = 0; t + l < h; ++t) acc = fma(e[t], e[t + l], acc);
            tab[LR_RANK_TAB_HEAD + l] += acc / (double)h;
        }
    }
}

int lr_rank_result(lr_rank *r, double *table, int64_t *n_draws) {
    if (!r || !table) return fail(LR_ERR_INVALID, "lr_rank_result: accumulator / table is NULL");
    const int p = r->p;
    if (n_draws) *n_draws = r->n;
    for (int i = 0; i < LR_RANK_ROWS * p; ++i) table[i] = NAN;
    if (r->n < 4) {
        for (int j = 0; j < p; ++j) table[11 * p + j] = 0.0;
        return LR_OK;
    }
    const int64_t h = r->n / 2, M = 2 * r->C, S = h * M, h2 = 2 * h;
    const int L = (int)(r->K < h - 1 ? r->K : h - 1);
    uint64_t *U = (uint64_t *)malloc((size_t)S * 8), *Ks = (uint64_t *)malloc((size_t)S * 8);
    int64_t *r2 = (int64_t *)malloc((size_t)S * 8);
    double *V = (double *)malloc((size_t)S * 8 * 4), *e = (double *)malloc((size_t)h * 8), *tab = (double *)malloc((size_t)(L + 3) * 8);
    if (!U || !Ks || !r2 || !V || !e || !tab) {
        free(U), free(Ks), free(r2), free(V), free(e), free(tab);
        return fail(LR_ERR_NOMEM, "lr_rank_result: workspace");
    }
    for (int j = 0; j < p; ++j) {
        rk_keys(r, j, S, 0, 0.0, U, Ks);
        const double med = (lr_rank_unkey(Ks[S / 2 - 1]) + lr_rank_unkey(Ks[S / 2])) * 0.5;
        const uint64_t k05 = Ks[(S - 1) / 20], k95 = Ks[19 * (S - 1) / 20];
        const int64_t bad = rk_bound(Ks, S, LR_RANK_KEY_NEG_INF, 1) + (S - rk_bound(Ks, S, LR_RANK_KEY_POS_INF, 0));
        table[11 * p + j] = (double)bad;
        if (bad) continue;
        table[8 * p + j] = med, table[9 * p + j] = lr_rank_unkey(k05), table[10 * p + j] = lr_rank_unkey(k95);
        rk_rank(U, Ks, S, r2);
        for (int64_t i = 0; i < S; ++i) {
            const int64_t t = i / r->C, c = i % r->C, o = c * h2 + t;
            V[o] = lr_rank_z(r2[i], S);
            V[2 * S + o] = U[i] <= k05 ? 1.0 : 0.0;
            V[3 * S + o] = U[i] <= k95 ? 1.0 : 0.0;
        }
        rk_keys(r, j, S, 1, med, U, Ks);
        rk_rank(U, Ks, S, r2);
        for (int64_t i = 0; i < S; ++i) V[S + (i % r->C) * h2 + i / r->C] = lr_rank_z(r2[i], S);
        double rhat[4], ess[4], capped[4], pairs[4];
        for (int s = 0; s < 4; ++s) {
            rk_table(V + (size_t)s * S, h, M, s == 1 ? 0 : L, tab, e);
            lr_rank_series(tab, h, M, s == 1 ? 0 : L, r->K, s != 1, &rhat[s], &ess[s], &capped[s], &pairs[s]);
        }
        table[0 * p + j] = rhat[0], table[1 * p + j] = rhat[1];
        table[2 * p + j] = isnan(rhat[0]) || isnan(rhat[1]) ? NAN : fmax(rhat[0], rhat[1]);
        table[3 * p + j] = ess[0];
        table[4 * p + j] = isnan(ess[2]) || isnan(ess[3]) ? NAN : fmin(ess[2], ess[3]);
        for (int i = 0; i < 3; ++i) table[(5 + i) * p + j] = capped[i ? i + 1 : 0], table[(12 + i) * p + j] = pairs[i ? i + 1 : 0];
    }
    free(U), free(Ks), free(r2), free(V), free(e), free(tab);
    return LR_OK;
}

int lr_rank_ranks(lr_rank *r, int32_t j, int32_t folded, int64_t *twice_r, double *z, int64_t *n_used) {
    if (!r || !twice_r) return fail(LR_ERR_INVALID, "lr_rank_ranks: accumulator / twice_r is NULL");
    if (j < 0 || j >= r->p) return fail(LR_ERR_INVALID, "lr_rank_ranks: coordinate %d is not in 0..%d", j, r->p - 1);
    if (n_used) *n_used = r->n / 2 * 2;
    if (r->n < 2) return LR_OK;
    const int64_t S = r->n / 2 * 2 * r->C;
    uint64_t *U = (uint64_t *)malloc((size_t)S * 8), *Ks = (uint64_t *)malloc((size_t)S * 8);
    if (!U || !Ks) {
        free(U), free(Ks);
        return fail(LR_ERR_NOMEM, "lr_rank_ranks: workspace");
    }
    rk_keys(r, j, S, 0, 0.0, U, Ks);
    if (folded) rk_keys(r, j, S, 1, (lr_rank_unkey(Ks[S / 2 - 1]) + lr_rank_unkey(Ks[S / 2])) * 0.5, U, Ks);
    rk_rank(U, Ks, S, twice_r);
    if (z)
        for (int64_t i = 0; i < S; ++i) z[i] = lr_rank_z(twice_r[i], S);
    free(U), free(Ks);
    return LR_OK;
}

int lr_rank_reset(lr_rank *r) {
    if (!r) return fail(LR_ERR_INVALID, "lr_rank_reset: accumulator is NULL");
    r->n = 0;
    return LR_OK;
}

void lr_rank_destroy(lr_rank *r) {
    if (!r) return;
    free(r->store);
    free(r);
}
