// lr_api.hip -- the entry points of the C ABI declared in include/logreg_hip.h: argument checking, model creation (device copies
// and operand images), the run / eval / plan calls and the device-memory helpers.  Host-side only.  The layers below it:
//   lr_model.h   the model handle, error reporting, variant tables, the dtype x width dispatch macros
//   lr_plan.h    which kernel variant runs a request (data): PlanReq is built by plan_request*(), planned by make_plan() / plan_run()
//   lr_engine.h  kernel argument packing, workspaces, the stepwise driver   lr_inst*.hip the launches, one unit per (dtype, width)
//   lr_accum.h   the scaffold of the accumulators of kept draws (the second half of this file, from the `posterior prediction` divider)
//   lr_adapt.h   the kernels of the NUTS warm-up (include/logreg_hip_adapt.h; its host side is the `NUTS warm-up` divider below)
// The first half has one of each: check_opts() for the options of every call, run_request() for the front every lr_run_* shares (check,
// plan_run(), nothing to do, device buffers or staged()), staged() for every call made with host pointers (run, NUTS, eval: allocate
// what the call uses, copy in, launch on the NULL stream, the only hipDeviceSynchronize of the run path, copy back), nuts_launch() for
// every NUTS launch (lr_run_nuts, lr_run_nuts_dense and each warm-up iteration: the metric and the tuning block are its data), and in
// lr_model_create one cleanup (a guard over lr_model_destroy), upload() for a device array and signed_rows() for the design, both
// shared with lr_predict_create.
// All arithmetic of the path runs in the kernels (lr_kernels.h, lr_mfma.h, lr_tall*.h, lr_wide*.h).
#include "../../include/logreg_hip.h"
#include "../../include/logreg_hip_nuts.h"
#include "../../include/logreg_hip_predict.h"
#include "../../include/logreg_hip_acf.h"
#include "../../include/logreg_hip_marginals.h"
#include "../../include/logreg_hip_loo.h"
#include "../../include/logreg_hip_cov.h"
#include "../../include/logreg_hip_adapt.h"
#include "../../include/logreg_hip_adapt_tall.h"
#include "../../include/logreg_hip_dense.h"
#include "../../include/logreg_hip_pg.h"
#include "../../include/logreg_hip_hs.h"
#include "../../include/logreg_hip_bridge.h"
#include "../../include/logreg_hip_rank.h"
#include "../../include/logreg_hip_ppc.h"

#include <hip/hip_runtime.h>
#define LR_STAMPS_HOST  // this unit also gets the host side of the development instrumentation (lr_stamps.h: empty in production builds)

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "lr_inst.h"
#include "lr_acf.h"
#include "lr_marginals.h"
#include "lr_cov.h"
#include "lr_kernels.h"
#include "lr_nuts.h"
#include "lr_nuts_dense.h"
#include "lr_pg.h"
#include "lr_hs.h"
#include "lr_dense.h"
#include "lr_adapt.h"
#include "lr_dense_adapt.h"
#include "lr_hessian.h"
#include "lr_mfma.h"
#include "lr_predict.h"
#include "lr_ppc.h"
#include "lr_loo.h"
#include "lr_bridge.h"
#include "lr_rank.h"
#include "lr_stats.h"
#include "lr_tall.h"
#include "lr_tall_nuts.h"
#include "lr_tall_mx.h"
#include "lr_wide_bf16.h"

#include "lr_model.h"

#include "lr_plan.h"
#include "lr_engine.h"
#include "lr_accum.h"

namespace {

int check_opts(const lr_model* m, const lr_run_opts* o, bool run) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!o) return fail(LR_ERR_INVALID, "opts is NULL");
    if (o->n_chains <= 0) return fail(LR_ERR_INVALID, "n_chains must be positive (got %lld)", (long long)o->n_chains);
    if (o->plan_chains < 0) return fail(LR_ERR_INVALID, "plan_chains must be 0 (= n_chains) or positive (got %d)", o->plan_chains);
    if (o->plan_chains > 0 && run && (o->plan_first < 0 || o->plan_first > o->chain_offset || o->chain_offset + o->n_chains > o->plan_first + o->plan_chains))
        return fail(LR_ERR_INVALID, "chains [%lld, %lld) are not inside the planned run [%lld, %lld) (plan_first, plan_chains)", (long long)o->chain_offset,
                    (long long)(o->chain_offset + o->n_chains), (long long)o->plan_first, (long long)(o->plan_first + o->plan_chains));
    if (const int rcg = check_group_for(m, o->group, o->mode)) return rcg;
    if (run) {
        if (o->thin <= 0 || o->iters < 0) return fail(LR_ERR_INVALID, "thin must be > 0 and iters >= 0");
        if (o->chain_offset < 0 || o->iter_offset < 0) return fail(LR_ERR_INVALID, "offsets must be >= 0");
        if ((uint64_t)(o->chain_offset + o->n_chains) > 0xFFFFFFFFull)
            return fail(LR_ERR_INVALID, "global chain ids must fit 32 bits");
        if (o->precision < LR_PREC_AUTO || o->precision > LR_PREC_BF16)
            return fail(LR_ERR_INVALID, "precision must be LR_PREC_AUTO/FULL/BF16");
        if (o->stats) {
            if (o->stats_batch < 1 || o->stats_first < 0 || o->stats_slots < 1)
                return fail(LR_ERR_INVALID, "stats needs stats_batch >= 1, stats_first >= 0, stats_slots >= 1");
            if (o->stats_first + o->iters > o->stats_slots * o->stats_batch)
                return fail(LR_ERR_INVALID, "stats buffer too small: kept samples %lld..%lld need more than %lld slots of %lld",
                            (long long)o->stats_first, (long long)(o->stats_first + o->iters), (long long)o->stats_slots,
                            (long long)o->stats_batch);
        }
    }
    return LR_OK;
}

// Host-pointer convenience path: stage through device buffers, run synchronously, copy back.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        if (bytes == 0) bytes = 1;
        return hipMalloc(&p, bytes) == hipSuccess ? 0 : -1;
    }
};
// One array of a call made with host pointers.  host = NULL: an optional array the caller left out -- nothing is allocated or copied
// and the launch gets NULL.
struct HostBuf {
    void* host;
    size_t bytes;
    bool in, out;  // copied to the device before the launch / back after it
};
// launch(d) enqueues on the NULL stream with d[i] the device copy of b[i]; the arrays come back only after a launch that worked
template <size_t N, typename Launch>
int staged(const HostBuf (&b)[N], Launch&& launch) {
    DevBuf d[N];
    void* dp[N];
    for (size_t i = 0; i < N; ++i) {
        if (b[i].host && d[i].alloc(b[i].bytes)) return fail(LR_ERR_NOMEM, "device allocation failed (array %zu of the call: %zu bytes)", i, b[i].bytes);
        dp[i] = d[i].p;
    }
    for (size_t i = 0; i < N; ++i)
        if (b[i].host && b[i].in) LR_HIP(hipMemcpy(dp[i], b[i].host, b[i].bytes, hipMemcpyHostToDevice));
    if (const int rc = launch(dp)) return rc;
    LR_HIP(hipDeviceSynchronize());
    for (size_t i = 0; i < N; ++i)
        if (b[i].host && b[i].out) LR_HIP(hipMemcpy(b[i].host, dp[i], b[i].bytes, hipMemcpyDeviceToHost));
    return LR_OK;
}

// The arrays of a run.  tally: accept counts (uint32 per chain), NUTS counters or Polya-Gamma counters, tally_item bytes per chain; launches add to it, so it
// is copied in as well as out.  lp_state: RWMH / MALA only.  depth_out: NUTS only.  aux (in/out, aux_item bytes per chain) and aux_out
// (aux_out_item bytes per chain and kept row): the horseshoe's hyper-state and its scale_out.
struct RunArrays {
    void* state;
    double* lp_state;
    void* out;
    void* tally;
    size_t tally_item;
    int8_t* depth_out;
    void* aux = nullptr;
    size_t aux_item = 0;
    void* aux_out = nullptr;
    size_t aux_out_item = 0;
};

// The front every lr_run_* shares, after the checks of its own parameters: check the options and arrays, plan, then either enqueue on
// the caller's stream over the caller's device buffers or stage host arrays (the statistics buffer is staged like the others, through a
// device-side view of the options).  launch(plan, stream, opts, arrays) is the family's launch.
template <typename Launch>
int run_request(lr_model* m, int kind, int max_depth, const lr_run_opts* o, const RunArrays& a, Launch&& launch) {
    int rc = check_opts(m, o, true);
    if (rc) return rc;
    if (!a.state) return fail(LR_ERR_INVALID, "state is NULL");
    if ((kind == LR_KIND_RWMH || kind == LR_KIND_MALA) && !a.lp_state) return fail(LR_ERR_INVALID, "lp_state is required for RWMH/MALA");
    LR_HIP(hipSetDevice(m->device));
    Plan pl;
    rc = plan_run(m, kind, o, max_depth, &pl);
    if (rc) return rc;
    if (o->iters == 0) return LR_OK;
    if (o->on_device) return launch(pl, (hipStream_t)o->stream, o, a);
    const size_t C = (size_t)o->n_chains, sbytes = C * m->p * m->esize();
    const HostBuf b[] = {{a.state, sbytes, true, true}, {a.lp_state, C * sizeof(double), true, true}, {a.out, (size_t)o->iters * sbytes, false, true},
                         {a.tally, C * a.tally_item, true, true}, {a.depth_out, (size_t)o->iters * C, false, true},
                         {o->stats, (size_t)o->stats_slots * C * 2 * m->p * sizeof(double), true, true},
                         {a.aux, C * a.aux_item, true, true}, {a.aux_out, (size_t)o->iters * C * a.aux_out_item, false, true}};
    return staged(b, [&](void* const* d) {
        lr_run_opts od = *o;
        od.stats = static_cast<double*>(d[5]);
        return launch(pl, nullptr, &od, RunArrays{d[0], static_cast<double*>(d[1]), d[2], d[3], a.tally_item, static_cast<int8_t*>(d[4]), d[6], a.aux_item, d[7], a.aux_out_item});
    });
}

int run_common(lr_model* m, const RunSpec& rs, const lr_run_opts* o, void* state, double* lp_state, void* out, uint32_t* accepts) {
    return run_request(m, rs.kind, 0, o, RunArrays{state, lp_state, out, accepts, sizeof(uint32_t), nullptr},
                       [&](const Plan& pl, hipStream_t st, const lr_run_opts* oo, const RunArrays& d) {
                           return do_chain(m, pl, st, rs, oo, d.state, d.lp_state, d.out, static_cast<uint32_t*>(d.tally));
                       });
}

static_assert(sizeof(lr::NutsCounters) == sizeof(lr_nuts_counters), "lr_nuts_counters layout");

// step and sqrt(dmm), eps / dmm, 1 / dmm of a diagonal metric, zero in padded coordinates: NutsArgs of a launch, the warm-up's NutsTune, HMC's RunSpec
template <typename T, int P>
void diag_tuning(int p, double eps, const double* dmm, T* step, T (&a)[P], T (&b)[P], T (&c)[P]) {
    *step = (T)eps;
    for (int j = 0; j < P; ++j) {
        a[j] = j < p ? (T)std::sqrt(dmm[j]) : T(0);
        b[j] = j < p ? (T)(eps / dmm[j]) : T(0);
        c[j] = j < p ? (T)(1.0 / dmm[j]) : T(0);
    }
}

// What differs between the NUTS launches, as data.  The metric: diagonal `dmm` (host), or a dense `factor` (device memory, lr_nuts_dense.h),
// or neither where the tuning block holds it.  The warm-up: `tune` (device, NutsTune: step, and the diagonal metric) and `astat` [C].
struct NutsMetric {
    const double* dmm;
    void* factor;
    void* tune;
    double* astat;
    const char* who;  // prefix of the launch's error text
};

// the NutsArgs base every variant shares, from the model, the options and the arrays
template <typename T, int P>
lr::NutsArgs<T, P> nuts_args(const lr_model* m, const lr_run_opts* o, int max_depth, const RunArrays& d) {
    lr::NutsArgs<T, P> na{};
    na.state = static_cast<T*>(d.state);
    na.out = static_cast<T*>(d.out);
    na.counters = static_cast<lr::NutsCounters*>(d.tally);
    na.depth_out = d.depth_out;
    na.C = o->n_chains;
    na.chain_offset = o->chain_offset;
    na.iters = o->iters;
    na.thin = o->thin;
    na.iter_offset = o->iter_offset;
    na.seed = o->seed;
    na.p = m->p;
    na.max_depth = max_depth;
    na.stats = lr::StatsArgs{o->stats, o->stats_batch, o->stats_first};
    return na;
}

// one NUTS launch of o->iters * o->thin iterations on `st`; every pointer of `d` and `mt` but dmm is device memory (eps: not read with mt.tune)
template <typename T, int P>
int nuts_launch(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, double eps, int max_depth, const NutsMetric& mt, const RunArrays& d) {
    auto ma = model_args<T, P>(m);
    lr::NutsArgs<T, P> na = nuts_args<T, P>(m, o, max_depth, d);
    if (mt.dmm) diag_tuning(m->p, eps, mt.dmm, &na.step, na.a, na.b, na.c);
    else if (!mt.tune) na.step = (T)eps;
    const auto* tune = static_cast<const lr::NutsTune<T, P>*>(mt.tune);
    const lr::NutsTunedArgs<T, P> tuned{na, tune, mt.astat};
    const lr::NutsDenseArgs<T, P> dense{na, static_cast<const T*>(mt.factor)};
    const lr::NutsDenseTunedArgs<T, P> dense_tuned{dense, tune, mt.astat};
    const void* const args[] = {&na, &tuned, &dense, &dense_tuned};  // by lr::NutsVariant
    const int variant = mt.factor ? (mt.tune ? lr::NUTS_DENSE_TUNED : lr::NUTS_DENSE) : (mt.tune ? lr::NUTS_DIAG_TUNED : lr::NUTS_DIAG);
    const lr::LaunchCfg cfg{pl.mode, pl.G, pl.R, LR_KIND_NUTS, st, pl.lds_bytes, m->dbg.residency_cap ? m->cus : 0};
    const int rc = m->table->launch_nuts(&cfg, o->n_chains, &ma, args[variant], variant);
    if (rc != 0) return fail(rc == -3 ? LR_ERR_UNSUPPORTED : LR_ERR_HIP, "%sNUTS launch failed (%d): %s", mt.who, rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}
int nuts_launch_any(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, double eps, int max_depth, const NutsMetric& mt, const RunArrays& d) {
    if (pl.mode == lr::MODE_STEPWISE) {  // (planned for the diagonal metric of lr_run_nuts only: plan_run)
        RunSpec rs{};
        rs.kind = lr::KIND_HMC;
        diag_tuning(m->p, eps, mt.dmm, &rs.step, rs.a, rs.b, rs.c);
        return do_nuts_stepwise(m, pl, st, rs, o, max_depth, d.state, d.out, d.tally, d.depth_out);
    }
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, nuts_launch, m, pl, st, o, eps, max_depth, mt, d)
    return bad_width(m);
}

// ---- NUTS under a dense metric (include/logreg_hip_dense.h; kernel: lr_nuts_dense.h, factorisation: lr_dense.h)
struct DenseFactorHost {
    std::vector<double> sigma;  // the lower triangle the factor was made from, row by row
    std::vector<unsigned char> image;  // lr_nuts_dense.h `factor` in the model's dtype
};
template <typename T, int P> int dense_image_t(int p, const double* s, const double* R, const double* A, std::vector<unsigned char>* img) {
    lr::dense_factor_image<T, P>(p, s, R, A, img);
    return LR_OK;
}
// factorise inv_metric for model m (no device access); LR_ERR_INVALID with the reason
int dense_factor_host(const lr_model* m, const char* who, const double* inv_metric, DenseFactorHost* f) {
    if (!inv_metric) return fail(LR_ERR_INVALID, "%s: inv_metric is NULL", who);
    if (m->P > 32) return fail(LR_ERR_UNSUPPORTED, "NUTS: p = %d > 32 -- wide models run on the stepwise engine, which has no NUTS kernel", m->p);
    const int p = m->p;
    std::vector<double> s((size_t)p), R((size_t)p * p), A((size_t)p * p);
    char why[200];
    if (lr::dense_factor(p, inv_metric, s.data(), R.data(), A.data(), why, sizeof(why))) return fail(LR_ERR_INVALID, "%s: %s", who, why);
    f->sigma.clear();
    for (int i = 0; i < p; ++i) f->sigma.insert(f->sigma.end(), inv_metric + (size_t)i * p, inv_metric + (size_t)i * p + i + 1);
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, dense_image_t, p, s.data(), R.data(), A.data(), &f->image)
    return bad_width(m);
}
// the device image of `f` for launches on `st`: the model keeps the last one per stream (lr_model.h `dense`); another factor on the same
// stream waits for the work enqueued there, which may still read the one it replaces
int dense_factor_device(lr_model* m, hipStream_t st, const DenseFactorHost& f, void** out) {
    lr_model::DenseFactor* slot = nullptr;
    for (auto& e : m->dense)
        if (e.stream == st) slot = &e;
    if (!slot) {
        if (m->dense.size() >= 16) {  // a caller cycling through streams (as the workspaces of lr_engine.h)
            LR_HIP(hipDeviceSynchronize());
            for (auto& e : m->dense)
                if (e.p) (void)hipFree(e.p);
            m->dense.clear();
        }
        void* p = nullptr;
        if (hipMalloc(&p, f.image.size()) != hipSuccess) return fail(LR_ERR_NOMEM, "device allocation failed (the dense metric's factor: %zu bytes)", f.image.size());
        m->dense.push_back({st, p, {}});
        slot = &m->dense.back();
    }
    if (slot->sigma != f.sigma) {
        LR_HIP(hipStreamSynchronize(st));
        slot->sigma.clear();  // (a failed copy leaves no claim on what the buffer holds)
        LR_HIP(hipMemcpy(slot->p, f.image.data(), f.image.size(), hipMemcpyHostToDevice));
        slot->sigma = f.sigma;
    }
    *out = slot->p;
    return LR_OK;
}

int positive_vec(const char* name, const double* v, int p) {
    if (!v) return fail(LR_ERR_INVALID, "%s is NULL", name);
    for (int j = 0; j < p; ++j)
        if (!(v[j] > 0) || !std::isfinite(v[j])) return fail(LR_ERR_INVALID, "%s[%d] must be finite and > 0", name, j);
    return LR_OK;
}

// The front lr_run_nuts and lr_run_nuts_dense share.  check() is the metric's own check, on the host, refused in this order: model, eps,
// max_depth, metric, then what run_request refuses; metric(stream, &mt) names the metric of the launch on that stream.
template <typename Check, typename Metric>
int run_nuts(lr_model* m, int kind, double eps, int max_depth, const lr_run_opts* o, void* state, void* out, lr_nuts_counters* counters, int8_t* depth_out, Check&& check,
             Metric&& metric) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!(eps > 0) || !std::isfinite(eps)) return fail(LR_ERR_INVALID, "eps must be finite and > 0");
    if (max_depth < 1 || max_depth > LR_NUTS_MAX_DEPTH) return fail(LR_ERR_INVALID, "max_depth must be in 1..%d (got %d)", LR_NUTS_MAX_DEPTH, max_depth);
    if (const int rc = check()) return rc;
    return run_request(m, kind, max_depth, o, RunArrays{state, nullptr, out, counters, sizeof(lr_nuts_counters), depth_out},
                       [&](const Plan& pl, hipStream_t st, const lr_run_opts* oo, const RunArrays& d) {
                           NutsMetric mt{nullptr, nullptr, nullptr, nullptr, ""};
                           if (const int rc = metric(st, &mt)) return rc;
                           return nuts_launch_any(m, pl, st, oo, eps, max_depth, mt, d);
                       });
}

// ---- Polya-Gamma Gibbs (include/logreg_hip_pg.h; kernel: lr_pg.h).  omega_out: lr_pg_omega (the draws of one sweep, nothing else written)
static_assert(sizeof(lr::PgCounters) == sizeof(lr_pg_counters) && LR_KIND_PG == lr::kKindPg && LR_PG_TAG == lr::TAG_PG &&
              LR_PG_MAX_ROUNDS == lr::kPgMaxRounds && LR_PG_MAX_TRIALS == lr::kPgMaxTrials && LR_PG_MAX_TERMS == lr::kPgMaxTerms, "logreg_hip_pg.h and lr_pg.h");
// the PgArgs of a launch, from the model, the options and the arrays
template <typename T, int P>
lr::PgArgs<T, P> pg_args(const lr_model* m, const lr_run_opts* o, const RunArrays& d, void* omega_out) {
    lr::PgArgs<T, P> pa{};
    pa.state = static_cast<T*>(d.state);
    pa.out = static_cast<T*>(d.out);
    pa.counters = static_cast<lr::PgCounters*>(d.tally);
    pa.omega_out = static_cast<T*>(omega_out);
    pa.C = o->n_chains;
    pa.chain_offset = o->chain_offset;
    pa.iters = o->iters;
    pa.thin = o->thin;
    pa.iter_offset = o->iter_offset;
    pa.seed = o->seed;
    pa.p = m->p;
    for (int j = 0; j < P; ++j) {
        pa.b[j] = j < m->p ? m->pg_b[(size_t)j] : 0.0;
        pa.ivar[j] = j < m->p ? m->inv_var[j] : 1.0;
    }
    pa.stats = lr::StatsArgs{o->stats, o->stats_batch, o->stats_first};
    return pa;
}
template <typename T, int P>
int pg_launch(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, const RunArrays& d, void* omega_out) {
    auto ma = model_args<T, P>(m);
    const lr::PgArgs<T, P> pa = pg_args<T, P>(m, o, d, omega_out);
    const lr::LaunchCfg cfg{pl.mode, pl.G, pl.R, LR_KIND_PG, st, pl.lds_bytes, m->dbg.residency_cap ? m->cus : 0};
    const int rc = m->table->launch_pg(&cfg, o->n_chains, &ma, &pa);
    if (rc != 0) return fail(rc == -3 ? LR_ERR_UNSUPPORTED : LR_ERR_HIP, "PG launch failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}
int pg_launch_any(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, const RunArrays& d, void* omega_out) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, pg_launch, m, pl, st, o, d, omega_out)
    return bad_width(m);
}

// ---- horseshoe Polya-Gamma Gibbs (include/logreg_hip_hs.h; kernel: lr_hs.h).  The prior as the kernel takes it; hyper_in != null:
// lr_hs_hyper (steps 5-7 of one iteration from hyper_in into d.aux, nothing else written)
static_assert(sizeof(lr_hs_counters) == sizeof(lr::PgCounters) && offsetof(lr_hs_counters, clamped) == offsetof(lr::PgCounters, reserved) &&
              LR_HS_TAG == lr::TAG_HS && LR_HS_BLOCK_GLOBAL == lr::kHsBlockGlobal && LR_HS_BLOCK_GAMMA == lr::kHsBlockGamma && LR_HS_MIN == lr::kHsLo &&
              LR_HS_MAX == lr::kHsHi, "logreg_hip_hs.h and lr_hs.h");
struct HsPrior {
    uint32_t shrink;
    int m;
    double inv_tau0sq;
};
template <typename T, int P>
int hs_launch(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, const RunArrays& d, const HsPrior& pr, const double* hyper_in) {
    auto ma = model_args<T, P>(m);
    lr::HsArgs<T, P> ha{};
    ha.pg = pg_args<T, P>(m, o, d, nullptr);
    ha.hyper_in = hyper_in ? hyper_in : static_cast<const double*>(d.aux);
    ha.hyper_out = static_cast<double*>(d.aux);
    ha.scale_out = static_cast<double*>(d.aux_out);
    ha.inv_tau0sq = pr.inv_tau0sq;
    ha.shrink = pr.shrink;
    ha.nexp = (pr.m + 1) / 2;
    ha.odd = (pr.m + 1) & 1;
    ha.hyper_only = hyper_in ? 1 : 0;
    const lr::LaunchCfg cfg{pl.mode, pl.G, pl.R, LR_KIND_PG, st, pl.lds_bytes, m->dbg.residency_cap ? m->cus : 0};
    const int rc = m->table->launch_hs(&cfg, o->n_chains, &ma, &ha);
    if (rc != 0) return fail(rc == -3 ? LR_ERR_UNSUPPORTED : LR_ERR_HIP, "horseshoe PG launch failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}
int hs_launch_any(lr_model* m, const Plan& pl, hipStream_t st, const lr_run_opts* o, const RunArrays& d, const HsPrior& pr, const double* hyper_in) {
    if (!m->table->launch_hs) return fail(LR_ERR_UNSUPPORTED, "horseshoe PG: no kernel for padded p = %d", m->P);
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, hs_launch, m, pl, st, o, d, pr, hyper_in)
    return bad_width(m);
}
// what lr_run_hs and lr_hs_hyper refuse about the prior and a hyper-state in host memory, ahead of any device access
int hs_check(const char* who, const lr_model* m, const lr_hs_prior* prior, const lr_run_opts* o, const double* hyper, const char* hyper_name, HsPrior* pr) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!prior) return fail(LR_ERR_INVALID, "%s: prior is NULL", who);
    if (!prior->shrink) return fail(LR_ERR_INVALID, "%s: prior->shrink is NULL", who);
    if (!(prior->global_scale > 0) || !std::isfinite(prior->global_scale)) return fail(LR_ERR_INVALID, "%s: global_scale must be finite and > 0", who);
    if (m->p > 32) return fail(LR_ERR_UNSUPPORTED, "PG: p = %d > 32 -- the Polya-Gamma kernel keeps a chain's p x p matrix on 16 lanes, up to p = 32", m->p);
    *pr = HsPrior{0u, 0, 1.0 / (prior->global_scale * prior->global_scale)};
    for (int j = 0; j < m->p; ++j)
        if (prior->shrink[j]) {
            pr->shrink |= 1u << j;
            ++pr->m;
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

// signed rows  xs_i = s_i x_i  of a design X [n][p], zero-padded to P columns, in the compute dtype;  s_i = 2 y_i - 1, or 1 without labels
// (`sign`, where given, receives them).  `name` is the caller's word for X in the message.
int signed_rows(const char* name, const double* X, const double* y, int64_t n, int p, int P, int dtype, std::vector<unsigned char>* host, signed char* sign) {
    host->resize((size_t)n * P * (dtype == LR_F32 ? 4 : 8));
    for (int64_t i = 0; i < n; ++i) {
        const double s = y ? 2.0 * y[i] - 1.0 : 1.0;
        if (sign) sign[i] = (signed char)s;
        for (int j = 0; j < P; ++j) {
            const double v = j < p ? s * X[i * p + j] : 0.0;
            if (!std::isfinite(v)) return fail(LR_ERR_INVALID, "%s[%lld,%d] is not finite", name, (long long)i, j);
            if (dtype == LR_F32) reinterpret_cast<float*>(host->data())[i * P + j] = (float)v;
            else reinterpret_cast<double*>(host->data())[i * P + j] = v;
        }
    }
    return LR_OK;
}

// One device array of a handle under construction: allocate, copy.  *dptr is the handle's field, so the handle's destroy call frees it
// whichever step fails.  copy_fail: the status of a failing copy (the operand images report LR_ERR_NOMEM for either step).
int upload(const char* who, const char* what, const void* host, size_t bytes, void** dptr, int copy_fail) {
    if (hipMalloc(dptr, bytes) != hipSuccess) return fail(LR_ERR_NOMEM, "%s: allocating the %s (%zu bytes) failed", who, what, bytes);
    const hipError_t e = hipMemcpy(*dptr, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(copy_fail, "%s: copying the %s (%zu bytes) failed: %s", who, what, bytes, hipGetErrorString(e));
    return LR_OK;
}

template <int P> size_t wide_block_elems() { return lr::WideBf16Geom<P>::BUF; }
template <int P> size_t wide_block1_elems() { return lr::WideBf16Geom<P>::BUF1; }

}  // namespace

// ------------------------------------------------------------------------------------------------
extern "C" {

const char* lr_last_error(void) { return g_err; }

#ifndef LR_BUILD_ID
#define LR_BUILD_ID "unversioned"
#endif
const char* lr_build_id(void) { return LR_BUILD_ID; }
int lr_sizeof_run_opts(void) { return (int)sizeof(lr_run_opts); }


int lr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lr_device_cus(int device) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(LR_ERR_HIP, "hipGetDeviceProperties failed");
    return prop.multiProcessorCount;
}

int lr_device_info(int device, char* buf, int len) {
    if (!buf || len <= 0) return fail(LR_ERR_INVALID, "NULL / empty buffer");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(LR_ERR_HIP, "hipGetDeviceProperties failed");
    char pci[32] = "?";
    if (hipDeviceGetPCIBusId(pci, sizeof pci, device) != hipSuccess) snprintf(pci, sizeof pci, "?");
    char uuid[33];
    for (int i = 0; i < 16; ++i) snprintf(uuid + 2 * i, 3, "%02x", (unsigned)(unsigned char)prop.uuid.bytes[i]);
    snprintf(buf, (size_t)len, "pci=%s uuid=%s name=%s cus=%d", pci, uuid, prop.name, prop.multiProcessorCount);
    return LR_OK;
}

int lr_model_create(const double* X, const double* y, int64_t n, int32_t p, const double* prior_sd, int32_t dtype,
                    int32_t device, lr_model** out) {
    if (!X || !y || !prior_sd || !out) return fail(LR_ERR_INVALID, "NULL argument");
    if (n <= 0 || p <= 0) return fail(LR_ERR_INVALID, "n and p must be positive");
    if (p > kMaxP) return fail(LR_ERR_UNSUPPORTED, "p=%d > %d is not supported", p, kMaxP);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "dtype must be LR_F32 or LR_F64");
    int rc = positive_vec("prior_sd", prior_sd, p);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (y[i] != 0.0 && y[i] != 1.0) return fail(LR_ERR_INVALID, "y[%lld]=%g is not 0/1", (long long)i, y[i]);
    int ndev = 0;
    LR_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(LR_ERR_HIP, "device %d not available (%d visible)", device, ndev);
    LR_HIP(hipSetDevice(device));

    std::unique_ptr<lr_model, decltype(&lr_model_destroy)> guard(new lr_model(), lr_model_destroy);  // every failure below destroys what exists
    lr_model* m = guard.get();
    m->device = device;
    char bad[64];
    if (!parse_debug_opts(std::getenv("LOGREG_DEBUG_OPTS"), &m->dbg, bad, sizeof bad))
        return fail(LR_ERR_INVALID, "LOGREG_DEBUG_OPTS: unknown or out-of-range item '%s' (keys: residency_cap=0|1, tall_mx16=0|1, "
                                    "wide_traj=0|1|2, wide_waves=4|8, wide_f16=0|1|2)", bad);
    m->dtype = dtype;
    m->n = n;
    m->p = p;
    m->P = padded_width(p);
    const int P = m->P;
    const ModelImages images = model_images(n, P, dtype);
    m->table = find_table(dtype, P);
    if (!m->table) return fail(LR_ERR_UNSUPPORTED, "no kernels for dtype=%d padded p=%d", dtype, P);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->cus = prop.multiProcessorCount;
    m->lprior_const = 0;
    for (int j = 0; j < kMaxP; ++j) m->inv_var[j] = 0;
    for (int j = 0; j < p; ++j) {
        m->inv_var[j] = 1.0 / (prior_sd[j] * prior_sd[j]);
        m->lprior_const += -std::log(prior_sd[j]) - 0.91893853320467274178;
    }
    const auto image = [](const char* what, const void* host, size_t bytes, void** dptr) { return upload("lr_model_create", what, host, bytes, dptr, LR_ERR_NOMEM); };
    std::vector<unsigned char> host;
    m->ysign.resize((size_t)n);
    if ((rc = signed_rows("X", X, y, n, p, P, dtype, &host, m->ysign.data()))) return rc;
    if ((rc = upload("lr_model_create", "rows", host.data(), host.size(), &m->d_rows, LR_ERR_HIP))) return rc;
    m->pg_b.assign((size_t)p, 0.0);  // X^T (y - 1/2) of the stored rows, summed in row order (include/logreg_hip_pg.h)
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < p; ++j)
            m->pg_b[(size_t)j] += dtype == LR_F32 ? (double)reinterpret_cast<const float*>(host.data())[i * P + j] : reinterpret_cast<const double*>(host.data())[i * P + j];
    for (int j = 0; j < p; ++j) m->pg_b[(size_t)j] *= 0.5;
    // the rows as float32, for the operand images (float64 models: rounded once, where an image is built from them)
    std::vector<float> rounded;
    if (dtype != LR_F32 && (images.tall_mx || images.wide1)) {
        const double* h64 = reinterpret_cast<const double*>(host.data());
        rounded.assign(h64, h64 + (size_t)n * P);
    }
    const float* hrows = dtype == LR_F32 ? reinterpret_cast<const float*>(host.data()) : rounded.data();
    if (P <= 32 && dtype == LR_F32) {
        // the rows once more as twisted row pairs, for the kernels that take them through the scalar unit:
        // pair k, coordinates (j, j+1), j even:  [k][j] = (A_j, B_{j+1}),  [k][j+1] = (A_{j+1}, B_j)  with
        // A = row 2k, B = row 2k+1 (a zero row closes an odd n)
        const int64_t npair = (n + 1) / 2;
        std::vector<float> tw((size_t)npair * P * 2, 0.0f);
        auto at = [&](int64_t r, int j) { return r < n ? hrows[r * P + j] : 0.0f; };
        for (int64_t k = 0; k < npair; ++k)
            for (int j = 0; j < P; j += 2) {
                float* q = tw.data() + ((size_t)k * P + j) * 2;
                q[0] = at(2 * k, j);
                q[1] = at(2 * k + 1, j + 1);
                q[2] = at(2 * k, j + 1);
                q[3] = at(2 * k + 1, j);
            }
        if ((rc = image("row-pair image", tw.data(), tw.size() * 4, &m->d_rows_tw))) return rc;
    }
    // narrow models the planner would ever send to the stepwise engine by itself (rows beyond 64 KB): two-piece bf16 tile images
    // for the interior HMC steps on the matrix pipe.  Smaller models run the engine only when forced (mode = STEPWISE), then in
    // fp32 throughout, and carry no image.
    if (images.tall_mx) {
        const int64_t ntile = (n + 31) / 32 * 2;
        std::vector<uint16_t> img((size_t)ntile * (P / 8) * lr::kMxSetElems);
        LR_BY_WIDTH_MX(P, lr::tall_mx_prepare, hrows, n, img.data());
        if ((rc = image("bf16 tile images", img.data(), img.size() * 2, &m->d_xmx))) return rc;
    }
    if (images.mf_end) {  // (up to 8192 rows: profiles/r2_midn_lds_mfma.txt)
        // the matrix-core chain kernel would keep its bf16 operands in LDS: fp32 operand images for its end points
        std::vector<float> img((size_t)((n + 15) / 16) * 64 * LR_BY_WIDTH_MX(P, lr::mf_image_floats));
        LR_BY_WIDTH_MX(P, lr::mf_image_prepare, hrows, n, img.data());
        if ((rc = image("fp32 operand images", img.data(), img.size() * 4, &m->d_xmf))) return rc;
        if (model_wants_xms(m) && m->table->mfma_image_bytes && m->table->launch_mfma_image) {
            const size_t ib = m->table->mfma_image_bytes(n);  // beyond LDS: the interior operands, built on the device once
            if (hipMalloc(&m->d_xms, ib) != hipSuccess || m->table->launch_mfma_image(nullptr, m->d_rows, n, m->d_xms) != 0 ||
                hipDeviceSynchronize() != hipSuccess)
                return fail(LR_ERR_NOMEM, "building the bf16 operand images (%zu bytes) failed", ib);
        }
    }
    const int64_t nblk = (n + 31) / 32;
    if (images.wide) {  // wide float32 models: bf16-piece block images for the exact-split matrix-core kernels
        std::vector<uint16_t> img((size_t)nblk * LR_BY_WIDTH_WIDE(P, wide_block_elems));
        LR_BY_WIDTH_WIDE(P, lr::wide_bf16_prepare, hrows, n, img.data());
        if ((rc = image("bf16 block images", img.data(), img.size() * 2, &m->d_xblk))) return rc;
    }
    if (images.wide1) {  // ... and the one-piece image (float64 models: from the rows rounded to float32)
        std::vector<uint16_t> img1((size_t)nblk * LR_BY_WIDTH_WIDE(P, wide_block1_elems));
        LR_BY_WIDTH_WIDE(P, lr::wide_bf16_prepare_rne, hrows, n, img1.data());
        if ((rc = image("single-piece bf16 block images", img1.data(), img1.size() * 2, &m->d_xblk1))) return rc;
        // the interior kernels' half-precision image, where the rows fit its range (lr_wide_bf16.h)
        if (LR_BY_WIDTH_WIDE(P, lr::wide_f16_prepare_rne, hrows, n, img1.data()))
            if ((rc = image("single-piece f16 block images", img1.data(), img1.size() * 2, &m->d_xblk1h))) return rc;
    }
    *out = guard.release();
    return LR_OK;
}

void lr_model_destroy(lr_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->d_rows) (void)hipFree(m->d_rows);
    if (m->d_rows_tw) (void)hipFree(m->d_rows_tw);
    for (auto& e : m->ws)
        if (e.p) (void)hipFree(e.p);
    for (auto& e : m->dense)
        if (e.p) (void)hipFree(e.p);
    if (m->d_xblk) (void)hipFree(m->d_xblk);
    if (m->d_xblk1) (void)hipFree(m->d_xblk1);
    if (m->d_xblk1h) (void)hipFree(m->d_xblk1h);
    if (m->d_xmx) (void)hipFree(m->d_xmx);
    if (m->d_xmf) (void)hipFree(m->d_xmf);
    if (m->d_xms) (void)hipFree(m->d_xms);
    for (auto& e : m->sides) {
        (void)hipStreamDestroy(e.stream);
        (void)hipEventDestroy(e.ev_fork);
        (void)hipEventDestroy(e.ev_join);
    }
    delete m;
}

int lr_model_debug_opts(const lr_model* m, char* buf, int len) {
    if (!m || !buf || len <= 0) return fail(LR_ERR_INVALID, "NULL argument / empty buffer");
    const DebugOpts& d = m->dbg;
    if (d.is_default()) snprintf(buf, (size_t)len, "%s", "");
    else snprintf(buf, (size_t)len, "residency_cap=%d,tall_mx16=%d,wide_traj=%d,wide_waves=%d,wide_f16=%d", d.residency_cap, d.tall_mx16, d.wide_traj, d.wide_waves, d.wide_f16);
    return LR_OK;
}

int lr_model_interior_format(const lr_model* m, int32_t* format) {
    if (!m || !format) return fail(LR_ERR_INVALID, "NULL argument");
    if (m->P > 32) *format = interior_f16(m) ? LR_INTERIOR_F16 : (m->d_xblk1 ? LR_INTERIOR_BF16 : LR_INTERIOR_NONE);
    else *format = m->P >= 8 ? LR_INTERIOR_BF16 : LR_INTERIOR_NONE;  // (the matrix-core kernels of lr_mfma.h / lr_mfma_f64.h / lr_tall_mx.h)
    return LR_OK;
}

int lr_model_info(const lr_model* m, int64_t* n, int32_t* p, int32_t* dtype, int32_t* device, int32_t* padded_p) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (n) *n = m->n;
    if (p) *p = m->p;
    if (dtype) *dtype = m->dtype;
    if (device) *device = m->device;
    if (padded_p) *padded_p = m->P;
    return LR_OK;
}

int lr_plan(const lr_model* m, int64_t n_chains, int32_t group, int32_t mode, int32_t* mode_out, int32_t* group_out,
            int32_t* rows_out) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (n_chains <= 0) return fail(LR_ERR_INVALID, "n_chains must be positive (got %lld)", (long long)n_chains);
    if (const int rcg = check_group_for(m, group, mode)) return rcg;
    Plan pl;
    const int rc = make_plan(plan_request(m, n_chains, group, mode), &pl);
    if (rc) return rc;
    if (mode_out) *mode_out = pl.mode;
    if (group_out) *group_out = pl.G;
    if (rows_out) *rows_out = pl.R;
    return LR_OK;
}

int lr_plan_run_info(const lr_model* m, int32_t kind, const lr_run_opts* o, lr_plan_info* out) {
    if (!out) return fail(LR_ERR_INVALID, "out is NULL");
    int rc = check_opts(m, o, false);
    if (rc) return rc;
    if ((kind < LR_KIND_RWMH || kind > LR_KIND_NUTS) && kind != LR_KIND_PG) return fail(LR_ERR_INVALID, "kind must be one of LR_KIND_*");
    Plan pl;
    rc = plan_run(m, kind, o, LR_NUTS_MAX_DEPTH, &pl);
    if (rc) return rc;
    *out = lr_plan_info{pl.mode, pl.G, pl.R, pl.G2, pl.R2, pl.split, pl.mode2, 0};
    return LR_OK;
}

int lr_plan_run(const lr_model* m, int32_t kind, const lr_run_opts* o, int32_t* mode_out, int32_t* group_out, int32_t* rows_out) {
    lr_plan_info pi;
    const int rc = lr_plan_run_info(m, kind, o, &pi);
    if (rc) return rc;
    if (mode_out) *mode_out = pi.mode;
    if (group_out) *group_out = pi.group;
    if (rows_out) *rows_out = pi.rows;
    return LR_OK;
}

int lr_eval(lr_model* m, const void* beta, void* ll, void* lprior, void* lpost, void* grad, const lr_run_opts* o) {
    int rc = check_opts(m, o, false);
    if (rc) return rc;
    if (!beta) return fail(LR_ERR_INVALID, "beta is NULL");
    LR_HIP(hipSetDevice(m->device));
    Plan pl;
    rc = make_plan(plan_request_eval(m, o), &pl);
    if (rc) return rc;
    const int64_t C = o->n_chains;
    if (o->on_device) return do_eval(m, pl, (hipStream_t)o->stream, C, beta, ll, lprior, lpost, grad);
    const size_t one = (size_t)C * m->esize(), vec = one * m->p;
    const HostBuf b[] = {{const_cast<void*>(beta), vec, true, false}, {ll, one, false, true}, {lprior, one, false, true}, {lpost, one, false, true},
                         {grad, vec, false, true}};
    return staged(b, [&](void* const* d) { return do_eval(m, pl, nullptr, C, d[0], d[1], d[2], d[3], d[4]); });
}

int lr_run_rwmh(lr_model* m, void* state, double* lp_state, const double* prop_sd, const lr_run_opts* o, void* out,
                uint32_t* accepts) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!prop_sd) return fail(LR_ERR_INVALID, "prop_sd is NULL");
    RunSpec rs{};
    rs.kind = lr::KIND_RWMH;
    for (int j = 0; j < m->p; ++j) {
        if (!(prop_sd[j] >= 0) || !std::isfinite(prop_sd[j])) return fail(LR_ERR_INVALID, "prop_sd[%d] must be finite and >= 0", j);
        rs.a[j] = prop_sd[j];
    }
    return run_common(m, rs, o, state, lp_state, out, accepts);
}

static int langevin_spec(lr_model* m, int kind, double dt, const double* pre, RunSpec* rs) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!(dt > 0) || !std::isfinite(dt)) return fail(LR_ERR_INVALID, "dt must be finite and > 0");
    const int rc = positive_vec("pre", pre, m->p);
    if (rc) return rc;
    rs->kind = kind;
    rs->step = dt;
    for (int j = 0; j < m->p; ++j) {
        rs->a[j] = 0.5 * pre[j] * dt;
        rs->b[j] = std::sqrt(pre[j]) * std::sqrt(dt);
        rs->c[j] = 1.0 / (rs->b[j] * rs->b[j]);
    }
    return LR_OK;
}

int lr_run_mala(lr_model* m, void* state, double* lp_state, double dt, const double* pre, const lr_run_opts* o, void* out,
                uint32_t* accepts) {
    RunSpec rs{};
    const int rc = langevin_spec(m, lr::KIND_MALA, dt, pre, &rs);
    if (rc) return rc;
    return run_common(m, rs, o, state, lp_state, out, accepts);
}

int lr_run_ul(lr_model* m, void* state, double dt, const double* pre, const lr_run_opts* o, void* out, uint32_t* accepts) {
    RunSpec rs{};
    const int rc = langevin_spec(m, lr::KIND_UL, dt, pre, &rs);
    if (rc) return rc;
    return run_common(m, rs, o, state, nullptr, out, accepts);
}

int lr_run_hmc(lr_model* m, void* state, double eps, int32_t l, const double* dmm, const lr_run_opts* o, void* out,
               uint32_t* accepts) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!(eps > 0) || !std::isfinite(eps)) return fail(LR_ERR_INVALID, "eps must be finite and > 0");
    if (l < 1) return fail(LR_ERR_INVALID, "l must be >= 1");
    const int rc = positive_vec("dmm", dmm, m->p);
    if (rc) return rc;
    RunSpec rs{};
    rs.kind = lr::KIND_HMC;
    rs.l = l;
    diag_tuning(m->p, eps, dmm, &rs.step, rs.a, rs.b, rs.c);
    return run_common(m, rs, o, state, nullptr, out, accepts);
}

// NUTS (include/logreg_hip_nuts.h; fit-blackjax-nuts.py:101, fit-numpyro.py:36-46).  opts->precision is read as FULL, lp_state does not
// exist, the run is one part (plan_nuts).
int lr_run_nuts(lr_model* m, void* state, double eps, int32_t max_depth, const double* dmm, const lr_run_opts* o, void* out,
                lr_nuts_counters* counters, int8_t* depth_out) {
    return run_nuts(m, LR_KIND_NUTS, eps, max_depth, o, state, out, counters, depth_out, [&] { return positive_vec("dmm", dmm, m->p); },
                    [&](hipStream_t, NutsMetric* mt) {
                        mt->dmm = dmm;
                        return LR_OK;
                    });
}

// NUTS under a dense metric (include/logreg_hip_dense.h): lr_run_nuts with the factor of inv_metric in place of dmm
int lr_dense_factor(int32_t p, const double* inv_metric, double* s, double* R, double* A) {
    if (!inv_metric) return fail(LR_ERR_INVALID, "lr_dense_factor: inv_metric is NULL");
    char why[200];
    if (lr::dense_factor(p, inv_metric, s, R, A, why, sizeof(why))) return fail(LR_ERR_INVALID, "lr_dense_factor: %s", why);
    return LR_OK;
}

int lr_run_nuts_dense(lr_model* m, void* state, double eps, int32_t max_depth, const double* inv_metric, const lr_run_opts* o, void* out,
                      lr_nuts_counters* counters, int8_t* depth_out) {
    DenseFactorHost f;
    return run_nuts(m, kKindNutsDense, eps, max_depth, o, state, out, counters, depth_out, [&] { return dense_factor_host(m, "lr_run_nuts_dense", inv_metric, &f); },
                    [&](hipStream_t st, NutsMetric* mt) {
                        mt->who = "dense ";
                        return dense_factor_device(m, st, f, &mt->factor);
                    });
}

// Polya-Gamma Gibbs (include/logreg_hip_pg.h; the tuning-free counterpart of R/fit-rjags.R).  opts->precision is not read, lp_state does
// not exist, the run is one part (plan_pg).
int lr_run_pg(lr_model* m, void* state, const lr_run_opts* o, void* out, lr_pg_counters* counters) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    return run_request(m, LR_KIND_PG, 0, o, RunArrays{state, nullptr, out, counters, sizeof(lr_pg_counters), nullptr},
                       [&](const Plan& pl, hipStream_t st, const lr_run_opts* oo, const RunArrays& d) { return pg_launch_any(m, pl, st, oo, d, nullptr); });
}

// the omega of one sweep at opts->iter_offset: the state is read, nothing but omega_out is written
int lr_pg_omega(lr_model* m, const void* state, const lr_run_opts* o, void* omega_out) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!o) return fail(LR_ERR_INVALID, "opts is NULL");
    if (!omega_out) return fail(LR_ERR_INVALID, "omega_out is NULL");
    lr_run_opts one = *o;  // (iters and thin are not read: one sweep)
    one.iters = 1;
    one.thin = 1;
    one.stats = nullptr;
    int rc = check_opts(m, &one, true);
    if (rc) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    LR_HIP(hipSetDevice(m->device));
    Plan pl;
    if ((rc = plan_run(m, LR_KIND_PG, &one, 0, &pl))) return rc;
    if (one.on_device) return pg_launch_any(m, pl, (hipStream_t)one.stream, &one, RunArrays{const_cast<void*>(state), nullptr, nullptr, nullptr, 0, nullptr}, omega_out);
    const size_t C = (size_t)one.n_chains;
    const HostBuf b[] = {{const_cast<void*>(state), C * m->p * m->esize(), true, false}, {omega_out, C * (size_t)m->n * m->esize(), false, true}};
    return staged(b, [&](void* const* d) { return pg_launch_any(m, pl, nullptr, &one, RunArrays{d[0], nullptr, nullptr, nullptr, 0, nullptr}, d[1]); });
}

// horseshoe Polya-Gamma Gibbs (include/logreg_hip_hs.h): lr_run_pg's request with the hyper-state and scale_out as two more arrays
int lr_run_hs(lr_model* m, const lr_hs_prior* prior, void* state, double* hyper, const lr_run_opts* o, void* out, double* scale_out, lr_hs_counters* counters) {
    HsPrior pr;
    if (const int rc = hs_check("lr_run_hs", m, prior, o, hyper, "hyper", &pr)) return rc;
    const size_t p = (size_t)m->p;
    return run_request(m, LR_KIND_PG, 0, o, RunArrays{state, nullptr, out, counters, sizeof(lr_hs_counters), nullptr, hyper, (2 * p + 2) * sizeof(double), scale_out, (p + 1) * sizeof(double)},
                       [&](const Plan& pl, hipStream_t st, const lr_run_opts* oo, const RunArrays& d) { return hs_launch_any(m, pl, st, oo, d, pr, nullptr); });
}

// steps 5-7 of the iteration at opts->iter_offset: state and hyper_in are read, hyper_out (and `clamped`) written
int lr_hs_hyper(lr_model* m, const lr_hs_prior* prior, const void* state, const double* hyper_in, const lr_run_opts* o, double* hyper_out, lr_hs_counters* counters) {
    HsPrior pr;
    if (const int rc0 = hs_check("lr_hs_hyper", m, prior, o, hyper_in, "hyper_in", &pr)) return rc0;
    if (!o) return fail(LR_ERR_INVALID, "opts is NULL");
    if (!hyper_out) return fail(LR_ERR_INVALID, "hyper_out is NULL");
    lr_run_opts one = *o;  // (iters and thin are not read: one iteration)
    one.iters = 1;
    one.thin = 1;
    one.stats = nullptr;
    int rc = check_opts(m, &one, true);
    if (rc) return rc;
    if (!state) return fail(LR_ERR_INVALID, "state is NULL");
    LR_HIP(hipSetDevice(m->device));
    Plan pl;
    if ((rc = plan_run(m, LR_KIND_PG, &one, 0, &pl))) return rc;
    const size_t C = (size_t)one.n_chains, hbytes = C * (2 * (size_t)m->p + 2) * sizeof(double);
    if (one.on_device)
        return hs_launch_any(m, pl, (hipStream_t)one.stream, &one, RunArrays{const_cast<void*>(state), nullptr, nullptr, counters, sizeof(lr_hs_counters), nullptr, hyper_out}, pr, hyper_in);
    const HostBuf b[] = {{const_cast<void*>(state), C * m->p * m->esize(), true, false}, {const_cast<double*>(hyper_in), hbytes, true, false}, {hyper_out, hbytes, false, true},
                         {counters, C * sizeof(lr_hs_counters), true, true}};
    return staged(b, [&](void* const* d) {
        return hs_launch_any(m, pl, nullptr, &one, RunArrays{d[0], nullptr, nullptr, d[3], sizeof(lr_hs_counters), nullptr, d[2]}, pr, static_cast<const double*>(d[1]));
    });
}

int lr_hessian(lr_model* m, const double* beta, double* lpost, double* grad, double* hess, void* stream) {
    if (!m) return fail(LR_ERR_INVALID, "model is NULL");
    if (!beta) return fail(LR_ERR_INVALID, "beta is NULL");
    LR_HIP(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const int p = m->p, NE = p * (p + 1) / 2, width = NE + p + 1;
    const int64_t nblocks = (m->n + lr::kHessRows - 1) / lr::kHessRows;
    DevBuf scratch;
    if (scratch.alloc(((size_t)nblocks * width + width + p) * sizeof(double))) return fail(LR_ERR_NOMEM, "lr_hessian scratch");
    double* d_part = static_cast<double*>(scratch.p);
    double* d_sums = d_part + (size_t)nblocks * width;
    double* d_beta = d_sums + width;
    LR_HIP(hipMemcpyAsync(d_beta, beta, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    const size_t lds = ((size_t)lr::kHessRows * p + 3 * lr::kHessRows + p) * sizeof(double);
    if (m->dtype == LR_F32)
        hipLaunchKernelGGL((lr::k_hess_partial<float>), dim3((unsigned)nblocks), dim3(256), lds, st,
                           static_cast<const float*>(m->d_rows), m->n, m->P, p, d_beta, d_part);
    else
        hipLaunchKernelGGL((lr::k_hess_partial<double>), dim3((unsigned)nblocks), dim3(256), lds, st,
                           static_cast<const double*>(m->d_rows), m->n, m->P, p, d_beta, d_part);
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_hess_final, dim3((width + 255) / 256), dim3(256), 0, st, d_part, nblocks, width, d_sums);
    LR_HIP(hipGetLastError());
    std::vector<double> h(width);
    LR_HIP(hipMemcpyAsync(h.data(), d_sums, (size_t)width * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    if (hess) {
        int e = 0;
        for (int a = 0; a < p; ++a)
            for (int c = a; c < p; ++c, ++e) hess[a * p + c] = hess[c * p + a] = h[e];
        for (int j = 0; j < p; ++j) hess[j * p + j] += m->inv_var[j];
    }
    if (grad)
        for (int j = 0; j < p; ++j) grad[j] = h[NE + j] - beta[j] * m->inv_var[j];
    if (lpost) {
        double quad = 0.0;
        for (int j = 0; j < p; ++j) quad += beta[j] * beta[j] * m->inv_var[j];
        *lpost = h[NE + p] + m->lprior_const - 0.5 * quad;
    }
    return LR_OK;
}

int lr_stats_reduce(int device, const double* stats, int64_t n_chains, int32_t p, int64_t batch, int64_t kept,
                    const double* pivot, double* sums, void* stream) {
    if (!stats || !pivot || !sums) return fail(LR_ERR_INVALID, "NULL argument");
    if (n_chains <= 0 || p <= 0 || p > kMaxP || batch < 1 || kept < 0)
        return fail(LR_ERR_INVALID, "lr_stats_reduce: need n_chains > 0, 0 < p <= %d, batch >= 1, kept >= 0", kMaxP);
    LR_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    int PW = 1;
    while (PW < p) PW *= 2;
    const int CY = 256 / PW;
    const int64_t nblocks = (n_chains + CY - 1) / CY;
    const size_t part_bytes = (size_t)nblocks * lr::kStatsRows * p * sizeof(double);
    const size_t tail_bytes = (size_t)(lr::kStatsRows + 1) * p * sizeof(double);  // final sums + the pivot
    DevBuf scratch;
    if (scratch.alloc(part_bytes + tail_bytes)) return fail(LR_ERR_NOMEM, "lr_stats_reduce scratch");
    double* d_part = static_cast<double*>(scratch.p);
    double* d_sums = d_part + (size_t)nblocks * lr::kStatsRows * p;
    double* d_piv = d_sums + (size_t)lr::kStatsRows * p;
    LR_HIP(hipMemcpyAsync(d_piv, pivot, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)nblocks), block(PW, CY);
    switch (PW) {
#define LR_STATS_CASE(W) \
    case W: hipLaunchKernelGGL((lr::k_stats_partial<W>), grid, block, 0, st, stats, n_chains, (int)p, batch, kept, d_piv, d_part); break;
        LR_STATS_CASE(1) LR_STATS_CASE(2) LR_STATS_CASE(4) LR_STATS_CASE(8) LR_STATS_CASE(16) LR_STATS_CASE(32)
        LR_STATS_CASE(64) LR_STATS_CASE(128)
#undef LR_STATS_CASE
    }
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_stats_final, dim3((lr::kStatsRows * p + 255) / 256), dim3(256), 0, st, d_part, nblocks, (int)p, d_sums);
    LR_HIP(hipGetLastError());
    LR_HIP(hipMemcpyAsync(sums, d_sums, (size_t)lr::kStatsRows * p * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

// ---- posterior prediction, pointwise log-likelihood (include/logreg_hip_predict.h; kernels: lr_predict.h) ----------------------------
}  // extern "C"
struct lr_predict : Staged {
    lr_model* m = nullptr;
    int device = 0;                 // the model's (kept here: lr_predict_destroy must not need the model)
    int64_t r = 0;
    bool labels = false;
    void* d_rows = nullptr;         // [r][P] signed rows in the model's dtype (the model's own d_rows when own_rows is false)
    bool own_rows = false;
    signed char* d_sign = nullptr;  // [r] 2 y - 1 (labels only)
    double* d_acc = nullptr;        // [LR_PRED_ROWS][r] the running table
    int64_t n = 0;                  // draws folded in
    Workspace part;                 // slice partials
};
namespace {
static_assert(LR_PRED_ROWS == lr::kPredRows, "table rows");

// slices of one launch over S draws: enough workgroups for four waves on every SIMD, at least 64 draws each
int64_t pred_most_slices(const lr_predict* pp, int64_t S) {  // non-decreasing in S
    const int64_t tiles = (pp->r + lr::kPredBlock - 1) / lr::kPredBlock;
    const int64_t want_blocks = (int64_t)(pp->m->cus > 0 ? pp->m->cus : 256) * 4;
    int64_t sl = (want_blocks + tiles - 1) / tiles;
    const int64_t most = (S + 63) / 64;
    if (sl > most) sl = most;
    return sl < 1 ? 1 : sl;
}
void pred_slicing(const lr_predict* pp, int64_t S, int64_t* per, int64_t* slices) {
    const int64_t sl = pred_most_slices(pp, S);
    *per = (S + sl - 1) / sl;
    *slices = (S + *per - 1) / *per;  // every slice non-empty
}

template <typename T, int P>
int pred_launch(lr_predict* pp, const void* d_draws, int64_t S, hipStream_t st) {
    int64_t per, slices;
    pred_slicing(pp, S, &per, &slices);
    const int64_t tiles = (pp->r + lr::kPredBlock - 1) / lr::kPredBlock;
    const size_t want = (size_t)slices * lr::kPredRows * pp->r * sizeof(double);
    if (const int rc = pp->part.grow(want, "lr_predict", "slice partials")) return rc;
    const dim3 grid((unsigned)tiles, (unsigned)slices);
    if (pp->labels)
        hipLaunchKernelGGL((lr::k_predict_partial<T, P, true>), grid, dim3(lr::kPredBlock), 0, st, static_cast<const T*>(pp->d_rows), pp->d_sign, pp->r,
                           static_cast<const T*>(d_draws), S, per, static_cast<double*>(pp->part.p));
    else
        hipLaunchKernelGGL((lr::k_predict_partial<T, P, false>), grid, dim3(lr::kPredBlock), 0, st, static_cast<const T*>(pp->d_rows), pp->d_sign, pp->r,
                           static_cast<const T*>(d_draws), S, per, static_cast<double*>(pp->part.p));
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_predict_merge, dim3((unsigned)((pp->r + lr::kPredMergeRows - 1) / lr::kPredMergeRows)),
                       dim3(lr::kPredMergeRows, lr::kPredMergeWays), 0, st, static_cast<const double*>(pp->part.p), slices, per, S, pp->r, (double)pp->n,
                       pp->d_acc);
    LR_HIP(hipGetLastError());
    pp->n += S;
    return LR_OK;
}
int pred_launch_any(lr_predict* pp, const void* d_draws, int64_t S, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, pp->m->dtype, pp->m->P, pred_launch, pp, d_draws, S, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_predict: unsupported padded width %d", pp->m->P);
}
}  // namespace
extern "C" {

int lr_predict_create(lr_model* m, const double* X_new, const double* y_new, int64_t r, lr_predict** out) {
    if (!m || !out) return fail(LR_ERR_INVALID, "lr_predict_create: model / out is NULL");
    if (r <= 0) return fail(LR_ERR_INVALID, "lr_predict_create: r must be positive (got %lld)", (long long)r);
    if (r > 0x7FFFFFFFll * lr::kPredMergeRows) return fail(LR_ERR_UNSUPPORTED, "lr_predict_create: r = %lld is beyond the launch grid", (long long)r);
    if (!X_new && y_new) return fail(LR_ERR_INVALID, "lr_predict_create: y_new without X_new (X_new = NULL means the model's own design AND labels)");
    if (!X_new && r != m->n) return fail(LR_ERR_INVALID, "lr_predict_create: X_new = NULL means the model's own %lld rows, r = %lld", (long long)m->n, (long long)r);
    if (y_new)
        for (int64_t i = 0; i < r; ++i)
            if (y_new[i] != 0.0 && y_new[i] != 1.0) return fail(LR_ERR_INVALID, "lr_predict_create: y_new[%lld]=%g is not 0/1", (long long)i, y_new[i]);
    LR_HIP(hipSetDevice(m->device));
    lr_predict* pp = new lr_predict();
    pp->m = m;
    pp->device = m->device;
    pp->r = r;
    pp->labels = !X_new || y_new;
    std::vector<signed char> sg;
    if (X_new) {
        std::vector<unsigned char> host;
        if (y_new) sg.resize((size_t)r);
        pp->own_rows = true;
        int rc = signed_rows("lr_predict_create: X_new", X_new, y_new, r, m->p, m->P, m->dtype, &host, y_new ? sg.data() : nullptr);
        if (!rc) rc = upload("lr_predict_create", "rows", host.data(), host.size(), &pp->d_rows, LR_ERR_HIP);
        if (rc) {
            lr_predict_destroy(pp);
            return rc;
        }
    } else {
        pp->d_rows = m->d_rows;
    }
    const std::vector<signed char>& signs = X_new ? sg : m->ysign;
    if (pp->labels)
        if (const int rc = upload("lr_predict_create", "labels", signs.data(), (size_t)r, (void**)&pp->d_sign, LR_ERR_HIP)) {
            lr_predict_destroy(pp);
            return rc;
        }
    if (hipMalloc((void**)&pp->d_acc, (size_t)LR_PRED_ROWS * r * sizeof(double)) != hipSuccess) {
        lr_predict_destroy(pp);
        return fail(LR_ERR_NOMEM, "lr_predict_create: allocating the table failed");
    }
    *out = pp;
    return LR_OK;
}

int lr_predict_accumulate(lr_predict* pp, const void* draws, int64_t S, int32_t on_device, void* stream) {
    if (!pp || !draws) return fail(LR_ERR_INVALID, "lr_predict_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_predict_accumulate: S must be positive (got %lld)", (long long)S);
    LR_HIP(hipSetDevice(pp->device));
    return stage_draws(
        "lr_predict", *pp, pp->m, Feed{draws, S, on_device != 0, (hipStream_t)stream},
        [pp](int64_t S0) { return pp->part.grow((size_t)pred_most_slices(pp, S0) * lr::kPredRows * pp->r * sizeof(double), "lr_predict", "slice partials"); },
        [pp](const void* d_draws, int64_t Sb, hipStream_t st) { return pred_launch_any(pp, d_draws, Sb, st); });
}

int lr_predict_result(lr_predict* pp, double* table, int64_t* n_draws) {
    if (!pp || !table) return fail(LR_ERR_INVALID, "lr_predict_result: accumulator / table is NULL");
    LR_HIP(hipSetDevice(pp->device));
    const size_t cells = (size_t)LR_PRED_ROWS * pp->r;
    if (pp->n > 0) {
        LR_HIP(hipMemcpyAsync(table, pp->d_acc, cells * sizeof(double), hipMemcpyDeviceToHost, pp->last));
        LR_HIP(hipStreamSynchronize(pp->last));
    }
    const size_t held = pp->n > 0 ? (pp->labels ? cells : 2 * (size_t)pp->r) : 0;  // (without labels: the two probability rows)
    fill_nan(table + held, cells - held);
    if (n_draws) *n_draws = pp->n;
    return LR_OK;
}

int lr_predict_reset(lr_predict* pp) {
    if (!pp) return fail(LR_ERR_INVALID, "lr_predict_reset: accumulator is NULL");
    pp->n = 0;  // the next merge starts the table afresh without reading it
    return LR_OK;
}

void lr_predict_destroy(lr_predict* pp) {
    if (!pp) return;
    (void)hipSetDevice(pp->device);
    if (pp->own_rows && pp->d_rows) (void)hipFree(pp->d_rows);
    free_all({pp->d_sign, pp->d_acc, pp->part.p, pp->in.p, pp->padded.p});
    delete pp;
}

// ---- posterior predictive checks from replicated outcomes (include/logreg_hip_ppc.h; kernels: lr_ppc.h) --------------------------------
}  // extern "C"
struct lr_ppc : Staged {
    lr_model* m = nullptr;
    int device = 0;
    int64_t r = 0;
    int G = 1;
    bool labels = false;
    uint64_t seed = 0;
    void* d_rows = nullptr;          // [r][P] signed rows (the model's own d_rows when own_rows is false)
    bool own_rows = false;
    signed char* d_sign = nullptr;   // [r] 2 y - 1 (labels only)
    unsigned char* d_grp = nullptr;  // [r] group labels (G > 1 only)
    int64_t* d_off = nullptr;        // [G] where group g's run of hist starts
    unsigned long long* d_tab = nullptr;  // hist [r + G] | row_ones [r] | counts [2]
    double* d_mom = nullptr;         // [lr::kPpcState] the running moments
    std::vector<int64_t> n_g, t_obs;
    int64_t n = 0;                   // draws handed over = the index s of the next one
    Workspace part, flags, dev;      // per-tile partials, finite flags and (D_obs, D_rep) of one sub-batch
    size_t tab_cells() const { return (size_t)r + (size_t)G + (size_t)r + 2; }
    unsigned long long* row_ones() const { return d_tab + r + G; }
    unsigned long long* counts() const { return d_tab + 2 * r + G; }
};
namespace {
static_assert(LR_PPC_MAX_GROUPS == lr::kPpcMaxGroups && LR_PPC_TAG == lr::TAG_PPC && LR_PPC_MOMENTS == lr::kPpcState - 1, "logreg_hip_ppc.h and lr_ppc.h");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the integer tables are 64-bit words");

constexpr size_t kPpcPartBytes = size_t(64) << 20;  // the most the per-tile partials of one sub-batch take (where four draws fit in it)
constexpr int64_t kPpcMostSub = int64_t(1) << 20;
int64_t ppc_tiles(int64_t r) { return (r + lr::kPpcBlock - 1) / lr::kPpcBlock; }
size_t ppc_part_per_draw(int64_t r, int G) { return (size_t)ppc_tiles(r) * (2 * sizeof(double) + (size_t)G * sizeof(uint32_t)); }
// The draws of one sub-batch: a function of (r, G) alone, a multiple of 4, at least 4.
int64_t ppc_sub_batch(int64_t r, int G) {
    const int64_t fit = (int64_t)(kPpcPartBytes / ppc_part_per_draw(r, G)) & ~int64_t(3);
    return std::min(kPpcMostSub, std::max<int64_t>(4, fit));
}
// the workspaces for pieces of at most S0 draws
int ppc_reserve(lr_ppc* pc, int64_t S0, bool terms) {
    const size_t nb = (size_t)std::min(S0, ppc_sub_batch(pc->r, pc->G));
    if (const int rc = pc->part.grow(nb * ppc_part_per_draw(pc->r, pc->G), "lr_ppc", "tile partials")) return rc;
    if (const int rc = pc->flags.grow(nb * sizeof(uint32_t), "lr_ppc", "finite flags")) return rc;
    return terms ? LR_OK : pc->dev.grow(nb * 2 * sizeof(double), "lr_ppc", "deviances");
}

struct PpcTerms {  // device outputs of lr_ppc_terms, and how many draws they hold already
    int32_t* counts;
    double* dev;
    uint32_t* yrep;
    int64_t words, done;
};

// S device-resident draws [S][P] whose first has the global index s0: sub-batch by sub-batch.  Every sub-batch but the last ends at a
// multiple of 4 of the global index, so a Philox block is never computed in two of them.
template <typename T, int P>
int ppc_launch(lr_ppc* pc, const void* d_draws, int64_t S, int64_t s0, PpcTerms* to, hipStream_t st) {
    const int64_t tiles = ppc_tiles(pc->r), sub = ppc_sub_batch(pc->r, pc->G), end = s0 + S;
    const int64_t want_blocks = (int64_t)(pc->m->cus > 0 ? pc->m->cus : 256) * 4;
    for (int64_t b = s0; b < end;) {
        const int64_t e = std::min(end, (b + sub) & ~int64_t(3)), nb = e - b;
        const T* d = static_cast<const T*>(d_draws) + (size_t)(b - s0) * P;
        uint32_t* flags = static_cast<uint32_t*>(pc->flags.p);
        double* part_d = static_cast<double*>(pc->part.p);
        uint32_t* part_c = reinterpret_cast<uint32_t*>(part_d + (size_t)tiles * nb * 2);
        hipLaunchKernelGGL(lr::k_ppc_flag<T>, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, d, nb, P, flags);
        LR_HIP(hipGetLastError());
        const int64_t span = e - (b & ~int64_t(3));
        int64_t sl = std::max<int64_t>(1, std::min((want_blocks + tiles - 1) / tiles, (span + 63) / 64));
        const int64_t per = ((span + sl - 1) / sl + 3) & ~int64_t(3);
        sl = (span + per - 1) / per;  // every slice non-empty
        const dim3 grid((unsigned)tiles, (unsigned)sl);
        unsigned long long* ones = to ? nullptr : pc->row_ones();
        uint32_t* yrep = to && to->yrep ? to->yrep + (size_t)to->done * to->words : nullptr;
        const int64_t words = to ? to->words : 0;
        if (pc->labels)
            hipLaunchKernelGGL((lr::k_ppc_partial<T, P, true>), grid, dim3(lr::kPpcBlock), 0, st, static_cast<const T*>(pc->d_rows), pc->d_sign, pc->d_grp, pc->r, pc->G, d,
                               flags, b, e, per, (uint32_t)pc->seed, (uint32_t)(pc->seed >> 32), part_d, part_c, ones, yrep, words);
        else
            hipLaunchKernelGGL((lr::k_ppc_partial<T, P, false>), grid, dim3(lr::kPpcBlock), 0, st, static_cast<const T*>(pc->d_rows), pc->d_sign, pc->d_grp, pc->r, pc->G, d,
                               flags, b, e, per, (uint32_t)pc->seed, (uint32_t)(pc->seed >> 32), part_d, part_c, ones, yrep, words);
        LR_HIP(hipGetLastError());
        double* dev = to ? to->dev + (size_t)to->done * 2 : static_cast<double*>(pc->dev.p);
        hipLaunchKernelGGL(lr::k_ppc_fold, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, part_d, part_c, flags, nb, tiles, pc->G, pc->labels ? 1 : 0, pc->d_off,
                           pc->d_tab, pc->counts(), dev, to ? to->counts + (size_t)to->done * pc->G : nullptr);
        LR_HIP(hipGetLastError());
        if (to) {
            to->done += nb;
        } else {
            hipLaunchKernelGGL(lr::k_ppc_moments, dim3(1), dim3(lr::kPpcMomBlock), 0, st, dev, flags, nb, pc->d_mom);
            LR_HIP(hipGetLastError());
            pc->n += nb;
        }
        b = e;
    }
    return LR_OK;
}
int ppc_launch_any(lr_ppc* pc, const void* d_draws, int64_t S, int64_t s0, PpcTerms* to, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, pc->m->dtype, pc->m->P, ppc_launch, pc, d_draws, S, s0, to, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_ppc: unsupported padded width %d", pc->m->P);
}
}  // namespace
extern "C" {

int lr_ppc_create(lr_model* m, const double* X_new, const double* y_new, int64_t r, const int32_t* groups, int32_t G, uint64_t seed, lr_ppc** out) {
    if (!m || !out) return fail(LR_ERR_INVALID, "lr_ppc_create: model / out is NULL");
    if (r <= 0) return fail(LR_ERR_INVALID, "lr_ppc_create: r must be positive (got %lld)", (long long)r);
    if (r > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "lr_ppc_create: r = %lld is beyond the 32-bit row word of the random stream", (long long)r);
    if (G < 1 || G > LR_PPC_MAX_GROUPS) return fail(LR_ERR_INVALID, "lr_ppc_create: G must be 1 .. %d (got %d)", LR_PPC_MAX_GROUPS, G);
    if (!groups && G != 1) return fail(LR_ERR_INVALID, "lr_ppc_create: groups = NULL means one group, G = %d", G);
    if (!X_new && y_new) return fail(LR_ERR_INVALID, "lr_ppc_create: y_new without X_new (X_new = NULL means the model's own design AND labels)");
    if (!X_new && r != m->n) return fail(LR_ERR_INVALID, "lr_ppc_create: X_new = NULL means the model's own %lld rows, r = %lld", (long long)m->n, (long long)r);
    if (y_new)
        for (int64_t i = 0; i < r; ++i)
            if (y_new[i] != 0.0 && y_new[i] != 1.0) return fail(LR_ERR_INVALID, "lr_ppc_create: y_new[%lld]=%g is not 0/1", (long long)i, y_new[i]);
    if (groups)
        for (int64_t i = 0; i < r; ++i)
            if (groups[i] < 0 || groups[i] >= G) return fail(LR_ERR_INVALID, "lr_ppc_create: groups[%lld]=%d is outside [0, %d)", (long long)i, groups[i], G);
    std::vector<unsigned char> host;
    std::vector<signed char> sg;
    if (X_new) {  // (non-finite X_new is refused here, ahead of any device access)
        if (y_new) sg.resize((size_t)r);
        if (const int rc = signed_rows("lr_ppc_create: X_new", X_new, y_new, r, m->p, m->P, m->dtype, &host, y_new ? sg.data() : nullptr)) return rc;
    }
    LR_HIP(hipSetDevice(m->device));
    lr_ppc* pc = new lr_ppc();
    pc->m = m;
    pc->device = m->device;
    pc->r = r;
    pc->G = G;
    pc->seed = seed;
    pc->labels = !X_new || y_new;
    const std::vector<signed char>& signs = X_new ? sg : m->ysign;
    pc->n_g.assign((size_t)G, 0);
    pc->t_obs.assign((size_t)G, pc->labels ? 0 : -1);
    std::vector<unsigned char> grp(groups && G > 1 ? (size_t)r : 0);
    for (int64_t i = 0; i < r; ++i) {
        const int g = groups ? groups[i] : 0;
        if (!grp.empty()) grp[(size_t)i] = (unsigned char)g;
        pc->n_g[(size_t)g] += 1;
        if (pc->labels && signs[(size_t)i] > 0) pc->t_obs[(size_t)g] += 1;
    }
    std::vector<int64_t> off((size_t)G, 0);
    for (int g = 1; g < G; ++g) off[(size_t)g] = off[(size_t)g - 1] + pc->n_g[(size_t)g - 1] + 1;
    int rc = LR_OK;
    if (X_new) {
        pc->own_rows = true;
        rc = upload("lr_ppc_create", "rows", host.data(), host.size(), &pc->d_rows, LR_ERR_HIP);
    } else {
        pc->d_rows = m->d_rows;
    }
    if (!rc && pc->labels) rc = upload("lr_ppc_create", "labels", signs.data(), (size_t)r, (void**)&pc->d_sign, LR_ERR_HIP);
    if (!rc && !grp.empty()) rc = upload("lr_ppc_create", "group labels", grp.data(), grp.size(), (void**)&pc->d_grp, LR_ERR_HIP);
    if (!rc) rc = upload("lr_ppc_create", "group offsets", off.data(), off.size() * sizeof(int64_t), (void**)&pc->d_off, LR_ERR_HIP);
    if (!rc && hipMalloc((void**)&pc->d_tab, pc->tab_cells() * sizeof(uint64_t)) != hipSuccess) rc = fail(LR_ERR_NOMEM, "lr_ppc_create: allocating the tables failed");
    if (!rc && hipMalloc((void**)&pc->d_mom, lr::kPpcState * sizeof(double)) != hipSuccess) rc = fail(LR_ERR_NOMEM, "lr_ppc_create: allocating the moments failed");
    if (!rc) rc = lr_ppc_reset(pc);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(LR_ERR_HIP, "lr_ppc_create: clearing the tables failed");
    if (rc) {
        lr_ppc_destroy(pc);
        return rc;
    }
    *out = pc;
    return LR_OK;
}

int lr_ppc_accumulate(lr_ppc* pc, const void* draws, int64_t S, int32_t on_device, void* stream) {
    if (!pc || !draws) return fail(LR_ERR_INVALID, "lr_ppc_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_ppc_accumulate: S must be positive (got %lld)", (long long)S);
    LR_HIP(hipSetDevice(pc->device));
    return stage_draws(
        "lr_ppc", *pc, pc->m, Feed{draws, S, on_device != 0, (hipStream_t)stream}, [pc](int64_t S0) { return ppc_reserve(pc, S0, false); },
        [pc](const void* d_draws, int64_t Sb, hipStream_t st) { return ppc_launch_any(pc, d_draws, Sb, pc->n, nullptr, st); });
}

int lr_ppc_terms(lr_ppc* pc, const void* draws, int64_t S, int64_t first_index, int32_t on_device, void* stream, int32_t* counts_out, double* dev_out,
                 uint32_t* yrep_out) {
    if (!pc || !draws || !counts_out || !dev_out) return fail(LR_ERR_INVALID, "lr_ppc_terms: accumulator / draws / counts_out / dev_out is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_ppc_terms: S must be positive (got %lld)", (long long)S);
    if (first_index < 0) return fail(LR_ERR_INVALID, "lr_ppc_terms: first_index must be >= 0 (got %lld)", (long long)first_index);
    LR_HIP(hipSetDevice(pc->device));
    const int64_t words = (pc->r + 31) / 32;
    const size_t b_dev = (size_t)S * 2 * sizeof(double), b_cnt = (size_t)S * pc->G * sizeof(int32_t), b_rep = yrep_out ? (size_t)S * words * sizeof(uint32_t) : 0;
    DevBuf buf;
    if (buf.alloc(b_dev + b_cnt + b_rep) != 0) return fail(LR_ERR_NOMEM, "lr_ppc_terms: allocating %zu bytes of output failed", b_dev + b_cnt + b_rep);
    unsigned char* base = static_cast<unsigned char*>(buf.p);
    PpcTerms to{reinterpret_cast<int32_t*>(base + b_dev), reinterpret_cast<double*>(base), yrep_out ? reinterpret_cast<uint32_t*>(base + b_dev + b_cnt) : nullptr, words, 0};
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = stage_draws(
            "lr_ppc", *pc, pc->m, Feed{draws, S, on_device != 0, st}, [pc](int64_t S0) { return ppc_reserve(pc, S0, true); },
            [pc, first_index, &to](const void* d_draws, int64_t Sb, hipStream_t s) { return ppc_launch_any(pc, d_draws, Sb, first_index + to.done, &to, s); })) {
        (void)hipStreamSynchronize(st);  // the output buffer is about to be freed
        return rc;
    }
    LR_HIP(hipMemcpyAsync(dev_out, to.dev, b_dev, hipMemcpyDeviceToHost, st));
    LR_HIP(hipMemcpyAsync(counts_out, to.counts, b_cnt, hipMemcpyDeviceToHost, st));
    if (yrep_out) LR_HIP(hipMemcpyAsync(yrep_out, to.yrep, b_rep, hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

int lr_ppc_result(lr_ppc* pc, uint64_t* hist, uint64_t* row_ones, uint64_t* counts, double* moments, int64_t* t_obs, int64_t* n_g, int64_t* n_draws) {
    if (!pc) return fail(LR_ERR_INVALID, "lr_ppc_result: accumulator is NULL");
    LR_HIP(hipSetDevice(pc->device));
    double state[lr::kPpcState];
    if (hist) LR_HIP(hipMemcpyAsync(hist, pc->d_tab, ((size_t)pc->r + pc->G) * sizeof(uint64_t), hipMemcpyDeviceToHost, pc->last));
    if (row_ones) LR_HIP(hipMemcpyAsync(row_ones, pc->row_ones(), (size_t)pc->r * sizeof(uint64_t), hipMemcpyDeviceToHost, pc->last));
    if (counts) LR_HIP(hipMemcpyAsync(counts, pc->counts(), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, pc->last));
    LR_HIP(hipMemcpyAsync(state, pc->d_mom, sizeof(state), hipMemcpyDeviceToHost, pc->last));
    LR_HIP(hipStreamSynchronize(pc->last));
    if (moments) {
        for (int k = 0; k < LR_PPC_MOMENTS; ++k) moments[k] = state[0] > 0.0 ? state[k + 1] : (double)NAN;
        if (!pc->labels) moments[0] = moments[1] = (double)NAN;
    }
    if (t_obs) std::copy(pc->t_obs.begin(), pc->t_obs.end(), t_obs);
    if (n_g) std::copy(pc->n_g.begin(), pc->n_g.end(), n_g);
    if (n_draws) *n_draws = pc->n;
    return LR_OK;
}

int lr_ppc_reset(lr_ppc* pc) {
    if (!pc) return fail(LR_ERR_INVALID, "lr_ppc_reset: accumulator is NULL");
    LR_HIP(hipSetDevice(pc->device));
    LR_HIP(hipMemsetAsync(pc->d_tab, 0, pc->tab_cells() * sizeof(uint64_t), pc->last));
    LR_HIP(hipMemsetAsync(pc->d_mom, 0, lr::kPpcState * sizeof(double), pc->last));
    pc->n = 0;
    return LR_OK;
}

void lr_ppc_destroy(lr_ppc* pc) {
    if (!pc) return;
    (void)hipSetDevice(pc->device);
    if (pc->own_rows && pc->d_rows) (void)hipFree(pc->d_rows);
    free_all({pc->d_sign, pc->d_grp, pc->d_off, pc->d_tab, pc->d_mom, pc->part.p, pc->flags.p, pc->dev.p, pc->in.p, pc->padded.p});
    delete pc;
}

// ---- autocorrelation and Geyer ESS of the kept draws (include/logreg_hip_acf.h; kernels: lr_acf.h) ------------------------------------
}  // extern "C"
struct lr_acf : Staged {
    int device = 0;
    int dtype = LR_F32;
    int64_t C = 0, NS = 0;  // chains, series = C p
    int p = 0, K = 0;
    int64_t n = 0;               // time steps folded in
    double* d_state = nullptr;   // S [NS][K+1] | head [NS][K] | tail [NS][K] | total [NS] | x0 [NS]
    size_t state_bytes = 0;
    Workspace ws;                // V, the workgroup partials and the table of lr_acf_result
    size_t esize() const { return dtype == LR_F32 ? 4 : 8; }
    double* S() const { return d_state; }
    double* head() const { return d_state + (size_t)NS * (K + 1); }
    double* tail() const { return head() + (size_t)NS * K; }
    double* total() const { return tail() + (size_t)NS * K; }
    double* x0() const { return total() + (size_t)NS; }
};
namespace {
static_assert(LR_ACF_MAX_LAG == lr::kAcfMaxLag, "largest lag");
static_assert(LR_ACF_ROWS(0) == lr::kAcfHeadRows + 1, "table rows");

template <typename T>
int acf_launch(lr_acf* a, const void* d_block, int64_t k, hipStream_t st) {
    const dim3 grid((unsigned)((a->NS + lr::kAcfTile - 1) / lr::kAcfTile)), blk(lr::kAcfBlock);
    const size_t lds = (size_t)lr::kAcfTile * lr::acf_row_doubles(a->K) * sizeof(double);
    const T* b = static_cast<const T*>(d_block);
    switch (a->K / 64 + 1) {  // lags per lane
#define LR_ACF_CASE(NL) \
    case NL: hipLaunchKernelGGL((lr::k_acf_accumulate<T, NL>), grid, blk, lds, st, b, k, a->NS, a->K, a->n, a->S(), a->total(), a->x0(), a->head(), a->tail()); break;
        LR_ACF_CASE(1) LR_ACF_CASE(2) LR_ACF_CASE(3) LR_ACF_CASE(4)
#undef LR_ACF_CASE
    }
    LR_HIP(hipGetLastError());
    a->n += k;
    return LR_OK;
}
}  // namespace
extern "C" {

int lr_acf_create(int device, int32_t dtype, int64_t C, int32_t p, int32_t max_lag, lr_acf** out) {
    if (!out) return fail(LR_ERR_INVALID, "lr_acf_create: out is NULL");
    if (C <= 0 || p <= 0) return fail(LR_ERR_INVALID, "lr_acf_create: C and p must be positive (got %lld, %d)", (long long)C, p);
    if (max_lag < 1 || max_lag > LR_ACF_MAX_LAG || max_lag % 2 == 0)
        return fail(LR_ERR_INVALID, "lr_acf_create: max_lag must be odd and in 1..%d (got %d)", LR_ACF_MAX_LAG, max_lag);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_acf_create: dtype must be LR_F32 or LR_F64");
    if (C > (0x7FFFFFFFll * lr::kAcfTile) / p) return fail(LR_ERR_UNSUPPORTED, "lr_acf_create: %lld x %d series are beyond the launch grid", (long long)C, p);
    if (const int rc = use_device(device, "lr_acf_create")) return rc;
    lr_acf* a = new lr_acf();
    a->device = device;
    a->dtype = dtype;
    a->C = C;
    a->p = p;
    a->K = max_lag;
    a->NS = C * p;
    a->state_bytes = (size_t)a->NS * (3 * (size_t)max_lag + 3) * sizeof(double);
    if (hipMalloc((void**)&a->d_state, a->state_bytes) != hipSuccess) {
        const size_t want = a->state_bytes;
        delete a;
        return fail(LR_ERR_NOMEM, "lr_acf_create: allocating %zu bytes of state failed", want);
    }
    hipError_t e = hipMemsetAsync(a->d_state, 0, a->state_bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        lr_acf_destroy(a);
        return fail(LR_ERR_HIP, "lr_acf_create: clearing the state failed: %s", hipGetErrorString(e));
    }
    *out = a;
    return LR_OK;
}

int lr_acf_accumulate(lr_acf* a, const void* block, int64_t k, int32_t on_device, void* stream) {
    if (!a || !block) return fail(LR_ERR_INVALID, "lr_acf_accumulate: accumulator / block is NULL");
    if (k <= 0) return fail(LR_ERR_INVALID, "lr_acf_accumulate: k must be positive (got %lld)", (long long)k);
    LR_HIP(hipSetDevice(a->device));
    return stage_block("lr_acf", *a, (size_t)a->NS * a->esize(), Feed{block, k, on_device != 0, (hipStream_t)stream},
                       [a](const void* d_block, int64_t kb, hipStream_t st) { return LR_BY_DTYPE(a->dtype, acf_launch, a, d_block, kb, st); });
}

int lr_acf_result(lr_acf* a, double* sums, double* ess_chain, int64_t* n_draws) {
    if (!a || !sums) return fail(LR_ERR_INVALID, "lr_acf_result: accumulator / sums is NULL");
    LR_HIP(hipSetDevice(a->device));
    const int64_t rows = LR_ACF_ROWS(a->K), cells = rows * a->p, nblocks = (a->C + 255) / 256;
    if (n_draws) *n_draws = a->n;
    if (a->n == 0) {
        fill_nan(sums, (size_t)cells);
        if (ess_chain) fill_nan(ess_chain, (size_t)a->NS);
        return LR_OK;
    }
    const size_t v_doubles = (size_t)rows * a->NS, part_doubles = (size_t)nblocks * cells;
    if (const int rc = a->ws.grow((v_doubles + part_doubles + (size_t)cells) * sizeof(double), "lr_acf", "result workspace")) return rc;
    double* V = static_cast<double*>(a->ws.p);
    double* part = V + v_doubles;
    double* d_sums = part + part_doubles;
    hipStream_t st = a->last;
    hipLaunchKernelGGL(lr::k_acf_finish, dim3((unsigned)((a->NS + 255) / 256)), dim3(256), 0, st, a->NS, a->K, a->n, a->S(), a->total(), a->head(), a->tail(), V);
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_acf_partial, dim3((unsigned)nblocks, (unsigned)rows), dim3(256), 0, st, V, a->C, a->p, part);
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_acf_final, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, part, nblocks, cells, d_sums);
    LR_HIP(hipGetLastError());
    LR_HIP(hipMemcpyAsync(sums, d_sums, (size_t)cells * sizeof(double), hipMemcpyDeviceToHost, st));
    if (ess_chain) LR_HIP(hipMemcpyAsync(ess_chain, V, (size_t)a->NS * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

int lr_acf_reset(lr_acf* a) {
    if (!a) return fail(LR_ERR_INVALID, "lr_acf_reset: accumulator is NULL");
    LR_HIP(hipSetDevice(a->device));
    LR_HIP(hipMemsetAsync(a->d_state, 0, a->state_bytes, a->last));
    LR_HIP(hipStreamSynchronize(a->last));
    a->n = 0;
    return LR_OK;
}

void lr_acf_destroy(lr_acf* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    free_all({a->d_state, a->in.p, a->ws.p});
    delete a;
}

// ---- rank-normalised split-R-hat, bulk and tail ESS of stored draws (include/logreg_hip_rank.h; kernels: lr_rank.h) ---------------------
}  // extern "C"
struct lr_rank : Staged {
    int device = 0;
    int dtype = LR_F32;
    int64_t C = 0, max_steps = 0;
    int p = 0, K = 0;
    int64_t n = 0;             // time steps stored
    void* d_store = nullptr;   // X [max_steps][C][p] in the draws' dtype
    Workspace ws;              // everything a result needs, for one batch of coordinates
    size_t esize() const { return dtype == LR_F32 ? 4 : 8; }
    size_t row() const { return (size_t)C * p * esize(); }
};
namespace {
static_assert(LR_RANK_MAX_LAG == lr::kRankMaxLag, "largest lag");
static_assert(LR_RANK_MAX_DRAWS / 2 <= 0x7FFFFFFFll, "a split chain per workgroup of the launch grid");

// How one batch of pb coordinates is laid out in the workspace (in 8-byte words), for n stored steps.
struct RankPlan {
    int64_t h, S, N, M, nblk;
    int L, rows, pb;
    size_t K, U, R, V, A, part, tab, Q, z, words;
    RankPlan(const lr_rank* r, int pb_, bool ranks) : pb(pb_) {
        h = r->n / 2;
        M = 2 * r->C;
        S = h * M;
        N = 2;
        while (N < S) N <<= 1;
        L = (int)std::min<int64_t>(r->K, h - 1);
        rows = L + 1 + LR_RANK_TAB_HEAD;
        nblk = (M + 255) / 256;
        size_t o = 0;
        const auto take = [&o](size_t w) { const size_t at = o; o += w; return at; };
        K = take((size_t)pb * N);
        U = take((size_t)pb * S);
        R = take((size_t)pb * S);
        V = take((size_t)lr::kRankSeries * pb * S);
        A = take((size_t)lr::kRankSeries * pb * (L + 2) * M);
        part = take((size_t)lr::kRankSeries * pb * rows * nblk);
        tab = take((size_t)lr::kRankSeries * pb * rows);
        Q = take((size_t)pb * lr::kRankQ);
        z = take(ranks ? (size_t)S : 0);
        words = o;
    }
};
// the most one batch of coordinates may take of device memory, and of the launch grid
constexpr size_t kRankBatchBytes = size_t(1) << 30;
constexpr int kRankBatchMax = 4096;

int rank_sort(uint64_t* K, int64_t N, int pb, hipStream_t st) {
    const unsigned tiles = (unsigned)std::max<int64_t>(1, N / lr::kRankTile);
    hipLaunchKernelGGL(lr::k_rank_sort_tile, dim3(tiles, pb), dim3(lr::kRankSortBlock), 0, st, K, N, (int64_t)0);
    LR_HIP(hipGetLastError());
    for (int64_t k = 2 * (int64_t)lr::kRankTile; k <= N; k <<= 1) {
        for (int64_t j = k >> 1; j >= lr::kRankTile; j >>= 1) {
            hipLaunchKernelGGL(lr::k_rank_merge_global, dim3((unsigned)((N / 2 + 255) / 256), pb), dim3(256), 0, st, K, N, k, j);
            LR_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(lr::k_rank_sort_tile, dim3(tiles, pb), dim3(lr::kRankSortBlock), 0, st, K, N, k);
        LR_HIP(hipGetLastError());
    }
    return LR_OK;
}

// Enqueue, for coordinates j0 .. j0 + pb of the stored draws: keys, sort, quantiles, and the passes `plain` / `fold` ask for (2r into R,
// z into V; the later pass overwrites R; z in time order where z_out is given).
template <typename T>
int rank_order(lr_rank* r, const RankPlan& P, int j0, bool plain, bool fold, double* z_out, hipStream_t st) {
    uint64_t* w = static_cast<uint64_t*>(r->ws.p);
    double* V = reinterpret_cast<double*>(w + P.V);
    int64_t* R = reinterpret_cast<int64_t*>(w + P.R);
    const dim3 gN((unsigned)((P.N + 255) / 256), P.pb), gS((unsigned)((P.S + 255) / 256), P.pb);
    hipLaunchKernelGGL(lr::k_rank_gather<T>, gN, dim3(256), 0, st, static_cast<const T*>(r->d_store), r->p, j0, P.S, P.N, w + P.U, w + P.K);
    LR_HIP(hipGetLastError());
    if (const int rc = rank_sort(w + P.K, P.N, P.pb, st)) return rc;
    hipLaunchKernelGGL(lr::k_rank_quant, dim3((unsigned)((P.pb + 63) / 64)), dim3(64), 0, st, w + P.K, P.S, P.N, P.pb, w + P.Q);
    LR_HIP(hipGetLastError());
    if (plain) {
        hipLaunchKernelGGL(lr::k_rank_lookup<false>, gS, dim3(256), 0, st, w + P.U, w + P.K, w + P.Q, P.S, P.N, R);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL(lr::k_rank_transform<false>, gS, dim3(256), 0, st, w + P.U, R, w + P.Q, r->C, 2 * P.h, P.S, V, fold ? nullptr : z_out);
        LR_HIP(hipGetLastError());
    }
    if (fold) {
        hipLaunchKernelGGL(lr::k_rank_fold, gN, dim3(256), 0, st, w + P.U, w + P.Q, P.S, P.N, w + P.K);
        LR_HIP(hipGetLastError());
        if (const int rc = rank_sort(w + P.K, P.N, P.pb, st)) return rc;
        hipLaunchKernelGGL(lr::k_rank_lookup<true>, gS, dim3(256), 0, st, w + P.U, w + P.K, w + P.Q, P.S, P.N, R);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL(lr::k_rank_transform<true>, gS, dim3(256), 0, st, w + P.U, R, w + P.Q, r->C, 2 * P.h, P.S, V, z_out);
        LR_HIP(hipGetLastError());
    }
    return LR_OK;
}

template <typename T>
int rank_batch(lr_rank* r, const RankPlan& P, int j0, double* h_tab, uint64_t* h_Q, hipStream_t st) {
    if (const int rc = rank_order<T>(r, P, j0, true, true, nullptr, st)) return rc;
    uint64_t* w = static_cast<uint64_t*>(r->ws.p);
    double* V = reinterpret_cast<double*>(w + P.V);
    double* A = reinterpret_cast<double*>(w + P.A);
    double* part = reinterpret_cast<double*>(w + P.part);
    double* tab = reinterpret_cast<double*>(w + P.tab);
    const int series = lr::kRankSeries * P.pb;
    const int64_t cells = (int64_t)series * P.rows;
    hipLaunchKernelGGL(lr::k_rank_lag, dim3((unsigned)P.M, series), dim3(256), 0, st, V, P.h, P.M, P.pb, P.L, A);
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_rank_partial, dim3((unsigned)P.nblk, P.rows, series), dim3(256), 0, st, A, P.M, part);
    LR_HIP(hipGetLastError());
    hipLaunchKernelGGL(lr::k_rank_final, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, part, P.nblk, cells, tab);
    LR_HIP(hipGetLastError());
    LR_HIP(hipMemcpyAsync(h_tab, tab, (size_t)cells * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipMemcpyAsync(h_Q, w + P.Q, (size_t)P.pb * lr::kRankQ * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

// rows of the result table of one coordinate, from its four series' tables and its quantiles
void rank_finish(const lr_rank* r, const RankPlan& P, const double* tab, const uint64_t* Q, int jb, int j, double* table) {
    const int p = r->p;
    const auto cell = [&](int row) -> double& { return table[(size_t)row * p + j]; };
    for (int row = 0; row < LR_RANK_ROWS; ++row) cell(row) = (double)NAN;
    const uint64_t* q = Q + (size_t)jb * lr::kRankQ;
    cell(11) = (double)q[3];
    if (q[3]) return;  // a NaN or an infinity among the draws
    for (int i = 0; i < 3; ++i) std::memcpy(&cell(8 + i), &q[i], sizeof(double));
    double rhat[4], ess[4], capped[4], pairs[4];
    for (int s = 0; s < lr::kRankSeries; ++s)
        lr_rank_series(tab + ((size_t)s * P.pb + jb) * P.rows, P.h, P.M, s == 1 ? 0 : P.L, r->K, s != 1, &rhat[s], &ess[s], &capped[s], &pairs[s]);
    cell(0) = rhat[0];
    cell(1) = rhat[1];
    cell(2) = std::isnan(rhat[0]) || std::isnan(rhat[1]) ? (double)NAN : std::max(rhat[0], rhat[1]);
    cell(3) = ess[0];
    cell(4) = std::isnan(ess[2]) || std::isnan(ess[3]) ? (double)NAN : std::min(ess[2], ess[3]);
    for (int i = 0; i < 3; ++i) {
        cell(5 + i) = capped[i ? i + 1 : 0];
        cell(12 + i) = pairs[i ? i + 1 : 0];
    }
}
}  // namespace
extern "C" {

int lr_rank_create(int device, int32_t dtype, int64_t C, int32_t p, int64_t max_steps, int32_t max_lag, lr_rank** out) {
    if (!out) return fail(LR_ERR_INVALID, "lr_rank_create: out is NULL");
    if (C <= 0 || p <= 0 || max_steps <= 0)
        return fail(LR_ERR_INVALID, "lr_rank_create: C, p and max_steps must be positive (got %lld, %d, %lld)", (long long)C, p, (long long)max_steps);
    if (max_lag < 1 || max_lag > LR_RANK_MAX_LAG || max_lag % 2 == 0)
        return fail(LR_ERR_INVALID, "lr_rank_create: max_lag must be odd and in 1..%d (got %d)", LR_RANK_MAX_LAG, max_lag);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_rank_create: dtype must be LR_F32 or LR_F64");
    if (C > LR_RANK_MAX_DRAWS || max_steps > LR_RANK_MAX_DRAWS / C)
        return fail(LR_ERR_UNSUPPORTED, "lr_rank_create: %lld chains x %lld steps are more than the cap of %lld draws per coordinate (LR_RANK_MAX_DRAWS)",
                    (long long)C, (long long)max_steps, (long long)LR_RANK_MAX_DRAWS);
    if (const int rc = use_device(device, "lr_rank_create")) return rc;
    lr_rank* r = new lr_rank();
    r->device = device;
    r->dtype = dtype;
    r->C = C;
    r->p = p;
    r->K = max_lag;
    r->max_steps = max_steps;
    const size_t want = (size_t)max_steps * r->row();
    if (hipMalloc(&r->d_store, want) != hipSuccess) {
        delete r;
        return fail(LR_ERR_NOMEM, "lr_rank_create: allocating %zu bytes for the draws failed", want);
    }
    *out = r;
    return LR_OK;
}

int lr_rank_accumulate(lr_rank* r, const void* block, int64_t k, int32_t on_device, void* stream) {
    if (!r || !block) return fail(LR_ERR_INVALID, "lr_rank_accumulate: accumulator / block is NULL");
    if (k <= 0) return fail(LR_ERR_INVALID, "lr_rank_accumulate: k must be positive (got %lld)", (long long)k);
    if (k > r->max_steps - r->n)
        return fail(LR_ERR_INVALID, "lr_rank_accumulate: %lld more steps after %lld exceed max_steps = %lld", (long long)k, (long long)r->n, (long long)r->max_steps);
    LR_HIP(hipSetDevice(r->device));
    return stage_block("lr_rank", *r, r->row(), Feed{block, k, on_device != 0, (hipStream_t)stream}, [r](const void* d_block, int64_t kb, hipStream_t st) {
        LR_HIP(hipMemcpyAsync(static_cast<unsigned char*>(r->d_store) + (size_t)r->n * r->row(), d_block, (size_t)kb * r->row(), hipMemcpyDeviceToDevice, st));
        r->n += kb;
        return (int)LR_OK;
    });
}

int lr_rank_result(lr_rank* r, double* table, int64_t* n_draws) {
    if (!r || !table) return fail(LR_ERR_INVALID, "lr_rank_result: accumulator / table is NULL");
    LR_HIP(hipSetDevice(r->device));
    if (n_draws) *n_draws = r->n;
    fill_nan(table, (size_t)LR_RANK_ROWS * r->p);
    if (r->n < 4) {
        std::fill(table + (size_t)11 * r->p, table + (size_t)12 * r->p, 0.0);
        return LR_OK;
    }
    const size_t per = RankPlan(r, 1, false).words * sizeof(uint64_t);
    const int pb = (int)std::max<size_t>(1, std::min<size_t>({(size_t)r->p, (size_t)kRankBatchMax, kRankBatchBytes / per}));
    const RankPlan P(r, pb, false);
    if (const int rc = r->ws.grow(P.words * sizeof(uint64_t), "lr_rank", "result workspace")) return rc;
    std::vector<double> h_tab;
    std::vector<uint64_t> h_Q;
    try {
        h_tab.resize((size_t)lr::kRankSeries * pb * P.rows);
        h_Q.resize((size_t)pb * lr::kRankQ);
    } catch (const std::bad_alloc&) {
        return fail(LR_ERR_NOMEM, "lr_rank_result: allocating the host tables failed");
    }
    for (int j0 = 0; j0 < r->p; j0 += pb) {
        // (a last batch of fewer coordinates runs as a full one on coordinates that end at p: the layout stays P's)
        const int jf = std::min(j0, r->p - pb);
        if (const int rc = LR_BY_DTYPE(r->dtype, rank_batch, r, P, jf, h_tab.data(), h_Q.data(), r->last)) return rc;
        for (int j = j0; j < std::min(r->p, j0 + pb); ++j) rank_finish(r, P, h_tab.data(), h_Q.data(), j - jf, j, table);
    }
    return LR_OK;
}

int lr_rank_ranks(lr_rank* r, int32_t j, int32_t folded, int64_t* twice_r, double* z, int64_t* n_used) {
    if (!r || !twice_r) return fail(LR_ERR_INVALID, "lr_rank_ranks: accumulator / twice_r is NULL");
    if (j < 0 || j >= r->p) return fail(LR_ERR_INVALID, "lr_rank_ranks: coordinate %d is not in 0..%d", j, r->p - 1);
    LR_HIP(hipSetDevice(r->device));
    if (n_used) *n_used = r->n / 2 * 2;
    if (r->n < 2) return LR_OK;
    const RankPlan P(r, 1, true);
    if (const int rc = r->ws.grow(P.words * sizeof(uint64_t), "lr_rank", "ranks workspace")) return rc;
    uint64_t* w = static_cast<uint64_t*>(r->ws.p);
    hipStream_t st = r->last;
    if (const int rc = LR_BY_DTYPE(r->dtype, rank_order, r, P, (int)j, !folded, folded != 0, z ? reinterpret_cast<double*>(w + P.z) : nullptr, st))
        return rc;
    LR_HIP(hipMemcpyAsync(twice_r, w + P.R, (size_t)P.S * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (z) LR_HIP(hipMemcpyAsync(z, w + P.z, (size_t)P.S * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

int lr_rank_reset(lr_rank* r) {
    if (!r) return fail(LR_ERR_INVALID, "lr_rank_reset: accumulator is NULL");
    LR_HIP(hipSetDevice(r->device));
    LR_HIP(hipStreamSynchronize(r->last));
    r->n = 0;
    return LR_OK;
}

void lr_rank_destroy(lr_rank* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    free_all({r->d_store, r->in.p, r->ws.p});
    delete r;
}

// ---- marginal histograms, min / max and power sums of the kept draws (include/logreg_hip_marginals.h; kernels: lr_marginals.h) ---------
}  // extern "C"
struct lr_marg : Staged {
    int device = 0;
    int dtype = LR_F32;
    int64_t C = 0, NS = 0;  // chains, series = C p
    int p = 0, bins = 0, pt = 0;  // pt: coordinates per LDS table (= p: the flat lane map)
    int64_t n = 0;               // time steps folded in
    unsigned long long* d_state = nullptr;  // counts [p][bins+3] | sums [NS][4] | mn [NS] | mx [NS] | grid [5][p], 8 bytes each
    Workspace ws;                // the workgroup partials and the table of lr_marg_result
    size_t esize() const { return dtype == LR_F32 ? 4 : 8; }
    int64_t cells() const { return (int64_t)p * LR_MARG_COLS(bins); }
    unsigned long long* counts() const { return d_state; }
    double* sums() const { return reinterpret_cast<double*>(d_state + cells()); }
    double* mn() const { return sums() + 4 * (size_t)NS; }
    double* mx() const { return mn() + (size_t)NS; }
    double* grid() const { return mx() + (size_t)NS; }
    size_t state_words() const { return (size_t)cells() + 6 * (size_t)NS + 5 * (size_t)p; }
};
namespace {
static_assert(LR_MARG_MAX_BINS == lr::kMargMaxBins, "most bins");
static_assert(LR_MARG_ROWS == lr::kMargRows, "table rows");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(double) == 8, "one state word is 8 bytes");
static_assert((size_t)lr::kMargBlock * lr::kMargMaxSteps < (size_t(1) << 32), "an LDS counter cannot wrap within a launch");

int marg_clear(lr_marg* m, hipStream_t st) {
    const int64_t most = std::max(m->cells(), m->NS);
    hipLaunchKernelGGL(lr::k_marg_init, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, m->NS, m->cells(), m->counts(), m->sums(), m->mn(), m->mx());
    LR_HIP(hipGetLastError());
    LR_HIP(hipStreamSynchronize(st));
    m->n = 0;
    return LR_OK;
}

template <typename T>
int marg_launch(lr_marg* m, const void* d_block, int64_t k, hipStream_t st) {
    int64_t blocks;
    if (m->pt == m->p) {
        blocks = (m->NS + lr::kMargBlock - 1) / lr::kMargBlock;
    } else {
        const int64_t per = lr::kMargBlock / m->pt;
        blocks = ((m->C + per - 1) / per) * ((m->p + m->pt - 1) / m->pt);
    }
    const size_t lds = (size_t)std::min(m->pt, m->p) * LR_MARG_COLS(m->bins) * sizeof(unsigned int);
    const T* b = static_cast<const T*>(d_block);
    for (int64_t t0 = 0; t0 < k; t0 += lr::kMargMaxSteps) {  // (an LDS counter takes at most 256 x kMargMaxSteps increments)
        const int64_t kb = std::min<int64_t>(lr::kMargMaxSteps, k - t0);
        hipLaunchKernelGGL((lr::k_marg_accumulate<T>), dim3((unsigned)blocks), dim3(lr::kMargBlock), lds, st, b + (size_t)t0 * m->NS, kb, m->C, m->p, m->bins,
                           m->pt, m->grid(), m->counts(), m->sums(), m->mn(), m->mx());
        LR_HIP(hipGetLastError());
    }
    m->n += k;
    return LR_OK;
}
}  // namespace
extern "C" {

int lr_marg_create(int device, int32_t dtype, int64_t C, int32_t p, int32_t bins, const double* lo, const double* hi, lr_marg** out) {
    if (!out || !lo || !hi) return fail(LR_ERR_INVALID, "lr_marg_create: out / lo / hi is NULL");
    if (C <= 0 || p <= 0) return fail(LR_ERR_INVALID, "lr_marg_create: C and p must be positive (got %lld, %d)", (long long)C, p);
    if (bins < 1 || bins > LR_MARG_MAX_BINS) return fail(LR_ERR_INVALID, "lr_marg_create: bins must be in 1..%d (got %d)", LR_MARG_MAX_BINS, bins);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_marg_create: dtype must be LR_F32 or LR_F64");
    for (int j = 0; j < p; ++j)
        if (!(std::isfinite(lo[j]) && std::isfinite(hi[j]) && lo[j] < hi[j] && std::isfinite(hi[j] - lo[j])))
            return fail(LR_ERR_INVALID, "lr_marg_create: the grid of coordinate %d must be finite with lo < hi (got %g, %g)", j, lo[j], hi[j]);
    const int pt = lr::marg_rows(p, bins);
    const int64_t per = pt == p ? 1 : lr::kMargBlock / pt, ntile = pt == p ? 1 : (p + pt - 1) / pt;
    if (C > 0x7FFFFFFFll * lr::kMargBlock / p || (C + per - 1) / per > 0x7FFFFFFFll / ntile)
        return fail(LR_ERR_UNSUPPORTED, "lr_marg_create: %lld x %d series are beyond the launch grid", (long long)C, p);
    if (const int rc = use_device(device, "lr_marg_create")) return rc;
    lr_marg* m = new lr_marg();
    m->device = device;
    m->dtype = dtype;
    m->C = C;
    m->p = p;
    m->bins = bins;
    m->pt = pt;
    m->NS = C * p;
    const size_t want = m->state_words() * 8;
    if (hipMalloc((void**)&m->d_state, want) != hipSuccess) {
        delete m;
        return fail(LR_ERR_NOMEM, "lr_marg_create: allocating %zu bytes of state failed", want);
    }
    std::vector<double> g(5 * (size_t)p);
    for (int j = 0; j < p; ++j) {
        g[j] = lo[j];
        g[(size_t)p + j] = (double)bins / (hi[j] - lo[j]);
        g[2 * (size_t)p + j] = (lo[j] + hi[j]) / 2.0;
        g[3 * (size_t)p + j] = 2.0 / (hi[j] - lo[j]);
        g[4 * (size_t)p + j] = hi[j];
    }
    hipError_t e = hipMemcpy(m->grid(), g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess || marg_clear(m, nullptr) != LR_OK) {
        lr_marg_destroy(m);
        return e != hipSuccess ? fail(LR_ERR_HIP, "lr_marg_create: copying the grid failed: %s", hipGetErrorString(e)) : LR_ERR_HIP;
    }
    *out = m;
    return LR_OK;
}

int lr_marg_accumulate(lr_marg* m, const void* block, int64_t k, int32_t on_device, void* stream) {
    if (!m || !block) return fail(LR_ERR_INVALID, "lr_marg_accumulate: accumulator / block is NULL");
    if (k <= 0) return fail(LR_ERR_INVALID, "lr_marg_accumulate: k must be positive (got %lld)", (long long)k);
    LR_HIP(hipSetDevice(m->device));
    return stage_block("lr_marg", *m, (size_t)m->NS * m->esize(), Feed{block, k, on_device != 0, (hipStream_t)stream},
                       [m](const void* d_block, int64_t kb, hipStream_t st) { return LR_BY_DTYPE(m->dtype, marg_launch, m, d_block, kb, st); });
}

int lr_marg_result(lr_marg* m, uint64_t* counts, double* table, int64_t* n_draws) {
    if (!m) return fail(LR_ERR_INVALID, "lr_marg_result: accumulator is NULL");
    LR_HIP(hipSetDevice(m->device));
    const int64_t tcells = (int64_t)LR_MARG_ROWS * m->p, nblocks = (m->C + 255) / 256;
    if (n_draws) *n_draws = m->n;
    if (m->n == 0) {
        if (counts) std::fill(counts, counts + m->cells(), uint64_t(0));
        if (table) fill_nan(table, (size_t)tcells);
        return LR_OK;
    }
    hipStream_t st = m->last;
    if (table) {
        if (const int rc = m->ws.grow((size_t)(nblocks + 1) * tcells * sizeof(double), "lr_marg", "result workspace")) return rc;
        double* part = static_cast<double*>(m->ws.p);
        double* d_table = part + (size_t)nblocks * tcells;
        hipLaunchKernelGGL(lr::k_marg_partial, dim3((unsigned)nblocks, (unsigned)LR_MARG_ROWS), dim3(256), 0, st, m->sums(), m->mn(), m->mx(), m->C, m->p, part);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL(lr::k_marg_final, dim3((unsigned)((tcells + 255) / 256)), dim3(256), 0, st, part, nblocks, m->p, d_table);
        LR_HIP(hipGetLastError());
        LR_HIP(hipMemcpyAsync(table, d_table, (size_t)tcells * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (counts) LR_HIP(hipMemcpyAsync(counts, m->counts(), (size_t)m->cells() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    if (table)
        for (int j = 0; j < m->p; ++j)
            if (table[j] > table[m->p + j]) table[j] = table[m->p + j] = NAN;  // +inf > -inf: the coordinate has no non-NaN draw
    return LR_OK;
}

int lr_marg_reset(lr_marg* m) {
    if (!m) return fail(LR_ERR_INVALID, "lr_marg_reset: accumulator is NULL");
    LR_HIP(hipSetDevice(m->device));
    return marg_clear(m, m->last);
}

void lr_marg_destroy(lr_marg* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    free_all({m->d_state, m->in.p, m->ws.p});
    delete m;
}

// ---- second cross-moment, chain sums of the kept draws (include/logreg_hip_cov.h; kernels: lr_cov.h) ------------------------------------
}  // extern "C"
struct lr_cov : Staged {
    int device = 0;
    int dtype = LR_F32;
    int64_t C = 0, G = 0, groups = 0;  // chains, chains per group, chain groups
    int p = 0, P = 0;
    int64_t n = 0;             // time steps folded in: the absolute time of the next block's first row
    double* d_state = nullptr;  // cells [groups R][E] | chain sums [C][p] | center [p] | scale [p]
    Workspace ws;              // the runs and the merged tables of lr_cov_result
    size_t esize() const { return dtype == LR_F32 ? 4 : 8; }
    int64_t E() const { return lr::cov_entries(P); }
    int64_t ncell() const { return groups * lr::cov_residues(P); }
    double* cells() const { return d_state; }
    double* chain_sums() const { return d_state + (size_t)(ncell() * E()); }
    double* cs() const { return chain_sums() + (size_t)C * p; }
    size_t sums_words() const { return (size_t)(ncell() * E()) + (size_t)C * p; }
};
namespace {
static_assert(LR_COV_CELL_RUN == lr::kCovCellRun && LR_COV_OUTER_RUN == lr::kCovOuterRun, "runs of the result");
template <int P>
constexpr bool cov_header_agrees() {
    return LR_COV_WIDTH(P) == P && LR_COV_RESIDUES(P) == lr::cov_residues(P) && LR_COV_CHUNK(P) == lr::cov_chunk(P) && LR_COV_GROUPS(P) == lr::cov_groups(P);
}
static_assert(cov_header_agrees<4>() && cov_header_agrees<8>() && cov_header_agrees<16>() && cov_header_agrees<32>() && cov_header_agrees<64>() &&
                  cov_header_agrees<128>() && LR_COV_WIDTH(LR_COV_MAX_P) == 128 && LR_COV_WIDTH(5) == 8 && LR_COV_WIDTH(1) == 4,
              "the partition the header states is the kernels'");

int cov_clear(lr_cov* h, hipStream_t st) {
    const int64_t count = (int64_t)h->sums_words();
    hipLaunchKernelGGL(lr::k_cov_init, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, h->d_state, count);
    LR_HIP(hipGetLastError());
    LR_HIP(hipStreamSynchronize(st));
    h->n = 0;
    return LR_OK;
}

template <typename T, int P>
int cov_launch(lr_cov* h, const void* d_block, int64_t k, hipStream_t st) {
    hipLaunchKernelGGL((lr::k_cov_accumulate<T, P>), dim3((unsigned)h->groups), dim3(lr::kCovBlock), 0, st, static_cast<const T*>(d_block), k, h->n, h->C, h->p, h->G,
                       h->cs(), h->cells(), h->chain_sums());
    LR_HIP(hipGetLastError());
    h->n += k;
    return LR_OK;
}
int cov_launch_any(lr_cov* h, const void* d_block, int64_t k, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, h->dtype, h->P, cov_launch, h, d_block, k, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_cov: unsupported padded width %d", h->P);
}
}  // namespace
extern "C" {

int lr_cov_create(int device, int32_t dtype, int64_t C, int32_t p, const double* center, const double* scale, lr_cov** out) {
    if (!out || !center || !scale) return fail(LR_ERR_INVALID, "lr_cov_create: out / center / scale is NULL");
    if (C <= 0 || p <= 0) return fail(LR_ERR_INVALID, "lr_cov_create: C and p must be positive (got %lld, %d)", (long long)C, p);
    if (p > LR_COV_MAX_P) return fail(LR_ERR_INVALID, "lr_cov_create: p must be in 1..%d (got %d)", LR_COV_MAX_P, p);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_cov_create: dtype must be LR_F32 or LR_F64");
    for (int j = 0; j < p; ++j)
        if (!(std::isfinite(center[j]) && std::isfinite(scale[j]) && scale[j] > 0))
            return fail(LR_ERR_INVALID, "lr_cov_create: coordinate %d needs a finite center and a finite scale > 0 (got %g, %g)", j, center[j], scale[j]);
    if (C > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "lr_cov_create: %lld chains are beyond the launch grid", (long long)C);
    if (const int rc = use_device(device, "lr_cov_create")) return rc;
    lr_cov* h = new lr_cov();
    h->device = device;
    h->dtype = dtype;
    h->C = C;
    h->p = p;
    h->P = LR_COV_WIDTH(p);
    h->G = lr::cov_group_chains(C, h->P);
    h->groups = (C + h->G - 1) / h->G;
    const size_t want = (h->sums_words() + 2 * (size_t)p) * sizeof(double);
    if (hipMalloc((void**)&h->d_state, want) != hipSuccess) {
        delete h;
        return fail(LR_ERR_NOMEM, "lr_cov_create: allocating %zu bytes of state failed", want);
    }
    std::vector<double> g(2 * (size_t)p);
    std::copy(center, center + p, g.begin());
    std::copy(scale, scale + p, g.begin() + p);
    hipError_t e = hipMemcpy(h->cs(), g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess || cov_clear(h, nullptr) != LR_OK) {
        lr_cov_destroy(h);
        return e != hipSuccess ? fail(LR_ERR_HIP, "lr_cov_create: copying center and scale failed: %s", hipGetErrorString(e)) : LR_ERR_HIP;
    }
    *out = h;
    return LR_OK;
}

int lr_cov_accumulate(lr_cov* h, const void* block, int64_t k, int32_t on_device, void* stream) {
    if (!h || !block) return fail(LR_ERR_INVALID, "lr_cov_accumulate: accumulator / block is NULL");
    if (k <= 0) return fail(LR_ERR_INVALID, "lr_cov_accumulate: k must be positive (got %lld)", (long long)k);
    LR_HIP(hipSetDevice(h->device));
    return stage_block("lr_cov", *h, (size_t)h->C * h->p * h->esize(), Feed{block, k, on_device != 0, (hipStream_t)stream},
                       [h](const void* d_block, int64_t kb, hipStream_t st) { return cov_launch_any(h, d_block, kb, st); });
}

int lr_cov_result(lr_cov* h, double* moment, double* chain_outer, double* sum, double* chain_sums, int64_t* n_draws) {
    if (!h) return fail(LR_ERR_INVALID, "lr_cov_result: accumulator is NULL");
    LR_HIP(hipSetDevice(h->device));
    const int p = h->p;
    const size_t pp = (size_t)p * p;
    if (n_draws) *n_draws = h->n;
    if (h->n == 0) {
        if (moment) fill_nan(moment, pp);
        if (chain_outer) fill_nan(chain_outer, pp);
        if (sum) fill_nan(sum, (size_t)p);
        if (chain_sums) fill_nan(chain_sums, (size_t)h->C * p);
        return LR_OK;
    }
    hipStream_t st = h->last;
    const int64_t E = h->E(), ncell = h->ncell(), F = (int64_t)pp + p;
    const int64_t mruns = (ncell + LR_COV_CELL_RUN - 1) / LR_COV_CELL_RUN, oruns = (h->C + LR_COV_OUTER_RUN - 1) / LR_COV_OUTER_RUN;
    const bool outer = chain_outer || sum;
    std::vector<double> tiles, full;
    if (moment || outer) {  // workspace: moment runs [mruns][E] | merged [E] | outer runs [oruns][F] | merged [F]
        const size_t words = (moment ? (size_t)(mruns + 1) * E : 0) + (outer ? (size_t)(oruns + 1) * F : 0);
        if (const int rc = h->ws.grow(words * sizeof(double), "lr_cov", "result workspace")) return rc;
        double* w = static_cast<double*>(h->ws.p);
        if (moment) {
            double* merged = w + (size_t)mruns * E;
            hipLaunchKernelGGL(lr::k_cov_runs, dim3((unsigned)((E + 255) / 256), (unsigned)mruns), dim3(256), 0, st, h->cells(), ncell, E, (int64_t)LR_COV_CELL_RUN, w);
            LR_HIP(hipGetLastError());
            hipLaunchKernelGGL(lr::k_cov_runs, dim3((unsigned)((E + 255) / 256), 1u), dim3(256), 0, st, w, mruns, E, mruns, merged);
            LR_HIP(hipGetLastError());
            tiles.resize((size_t)E);
            LR_HIP(hipMemcpyAsync(tiles.data(), merged, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
            w = merged + E;
        }
        if (outer) {
            double* merged = w + (size_t)oruns * F;
            hipLaunchKernelGGL(lr::k_cov_outer, dim3((unsigned)oruns, (unsigned)((F + 255) / 256)), dim3(256), 0, st, h->chain_sums(), h->C, p, w);
            LR_HIP(hipGetLastError());
            hipLaunchKernelGGL(lr::k_cov_runs, dim3((unsigned)((F + 255) / 256), 1u), dim3(256), 0, st, w, oruns, F, oruns, merged);
            LR_HIP(hipGetLastError());
            full.resize((size_t)F);
            LR_HIP(hipMemcpyAsync(full.data(), merged, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    if (chain_sums) LR_HIP(hipMemcpyAsync(chain_sums, h->chain_sums(), (size_t)h->C * p * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    if (moment) {  // tiles (bi <= bj, row-major) of T x T entries -> the full symmetric matrix
        const int T = lr::cov_tile(h->P), nb = lr::cov_nb(h->P);
        size_t tile = 0;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi; bj < nb; ++bj, ++tile)
                for (int a = 0; a < T; ++a)
                    for (int b = 0; b < T; ++b) {
                        const int i = bi * T + a, j = bj * T + b;
                        if (i <= j && j < p) moment[(size_t)i * p + j] = moment[(size_t)j * p + i] = tiles[tile * T * T + (size_t)a * T + b];
                    }
    }
    if (chain_outer)
        for (int i = 0; i < p; ++i)
            for (int j = i; j < p; ++j) chain_outer[(size_t)i * p + j] = chain_outer[(size_t)j * p + i] = full[(size_t)i * p + j];
    if (sum) std::copy(full.begin() + pp, full.end(), sum);
    return LR_OK;
}

int lr_cov_reset(lr_cov* h) {
    if (!h) return fail(LR_ERR_INVALID, "lr_cov_reset: accumulator is NULL");
    LR_HIP(hipSetDevice(h->device));
    return cov_clear(h, h->last);
}

void lr_cov_destroy(lr_cov* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    free_all({h->d_state, h->in.p, h->ws.p});
    delete h;
}

// ---- NUTS warm-up: pooled step-size and metric adaptation (include/logreg_hip_adapt.h; kernels: lr_nuts.h TUNED, lr_adapt.h) ---------------
}  // extern "C"
namespace {
// The dense metric of a warm-up (include/logreg_hip_dense.h "Warm-up"): the part of a handle that lr_dense_adapt_create adds, and the
// steps it adds to the loop of adapt_enqueue
struct DenseAdapt {
    void* d_factor = nullptr;         // lr_nuts_dense.h `factor` of sigma
    double* d_comoment = nullptr;     // with adapt_metric: the window's triple | the workgroups' triples [B] (lr_dense_adapt.h)
    std::vector<double> sigma;        // the current inverse metric [p][p]
    std::vector<double> sigma_trace;  // [n_windows][p][p]: Sigma after each window done
    int64_t skipped = 0;              // windows whose Sigma was refused (the previous metric stays)
    int windows = 0;
    ~DenseAdapt() { free_all({d_factor, d_comoment}); }  // (lr_adapt_destroy has set the device)

    // an iteration inside a window: the states [C][p] into the window's pooled co-moment (lr_dense_adapt.h), two launches on `st`
    template <typename T, int P> int accumulate(hipStream_t st, const void* state, int64_t C, int64_t B, int p) {
        double* part = d_comoment + lr::dense_triple_words(P);
        hipLaunchKernelGGL((lr::k_dense_comoment_partial<T, P>), dim3((unsigned)B), dim3(lr::kAdaptBlock), 0, st, static_cast<const T*>(state), C, p, part);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL((lr::k_dense_comoment_merge<P>), dim3(1), dim3(P * P < 64 ? 64 : P * P), 0, st, part, B, p, d_comoment);
        LR_HIP(hipGetLastError());
        return LR_OK;
    }
    // The end of a window (lr_dense_adapt.h: dense_window_end): the one host synchronisation of the warm-up.  Reads the window's pooled triple, forms S = M / (n - 1) and
    // Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I, factorises it and replaces the device factor; a Sigma that lr_dense_factor refuses keeps
    // the previous metric and is counted.  The triple is emptied for the next window.
    int window_end(const lr_model* m, hipStream_t st) {
        const int p = m->p, P = m->P;
        const size_t tw = (size_t)lr::dense_triple_words(P);
        std::vector<double> win(tw);
        LR_HIP(hipStreamSynchronize(st));
        LR_HIP(hipMemcpy(win.data(), d_comoment, tw * sizeof(double), hipMemcpyDeviceToHost));
        const double n = win[0];
        std::vector<double> sig((size_t)p * p);
        for (int j = 0; j < p; ++j)
            for (int l = 0; l <= j; ++l) {
                const double S = win[1 + P + (size_t)j * P + l] / (n - 1.0);
                const double v = (n / (n + 5.0)) * S + (j == l ? 1e-3 * (5.0 / (n + 5.0)) : 0.0);
                sig[(size_t)j * p + l] = sig[(size_t)l * p + j] = v;
            }
        DenseFactorHost f;
        if (dense_factor_host(m, "lr_dense_adapt_run", sig.data(), &f) == LR_OK) {
            LR_HIP(hipMemcpy(d_factor, f.image.data(), f.image.size(), hipMemcpyHostToDevice));
            sigma = sig;
        } else {
            ++skipped;
        }
        std::copy(sigma.begin(), sigma.end(), sigma_trace.begin() + (size_t)windows * p * p);
        ++windows;
        LR_HIP(hipMemsetAsync(d_comoment, 0, tw * sizeof(double), st));
        return LR_OK;
    }
};
}  // namespace
struct lr_adapt {
    lr_model* m = nullptr;
    int64_t C = 0, B = 0;  // chains, workgroups of k_adapt_partial
    int W = 0, n_windows = 0, init = 0;
    int ends[LR_ADAPT_MAX_WINDOWS] = {};
    double delta = 0.8, gamma = 0.05, t0 = 10.0, kappa = 0.75;
    int64_t t = 0;     // iterations enqueued
    int m_since = 0;   // ... of them since the last restart of dual averaging
    int window = 0;    // the first window that has not ended
    hipStream_t last = nullptr;  // stream of the last run call: results follow it
    bool failed = false;         // a launch failed part-way through a run call: what is enqueued no longer matches the counts above
    bool tall = false;           // lr_tall_adapt_create: the iterations run on the stepwise engine (include/logreg_hip_adapt_tall.h)
    // one device block: da | dmm [p] | window triple [1 + 2 p] | partials [B][2 + 2 P] | trace [W][5] | metric [windows][2][p] | astat [C] | NutsTune
    double* d_fixed = nullptr;
    size_t words = 0, tune_bytes = 0;
    Workspace st_state, st_out, st_tally, st_depth, st_astat;  // a call made with host pointers stages its arrays here
    std::unique_ptr<DenseAdapt> dense;  // lr_dense_adapt_create: the iterations run k_nuts_dense under dense->d_factor
    int p() const { return m->p; }
    size_t o_dmm() const { return 8; }
    size_t o_win() const { return o_dmm() + (size_t)p(); }
    size_t o_partial() const { return o_win() + 1 + 2 * (size_t)p(); }
    size_t o_trace() const { return o_partial() + (size_t)B * lr::adapt_partial_words(m->P); }
    size_t o_metric() const { return o_trace() + (size_t)W * LR_ADAPT_TRACE_COLS; }
    size_t o_astat() const { return o_metric() + (size_t)(n_windows > 0 ? n_windows : 1) * 2 * p(); }
    size_t o_tune() const { return o_astat() + (size_t)C; }
    lr::AdaptDev dev() const { return lr::AdaptDev{d_fixed, d_fixed + o_dmm(), d_fixed + o_win(), d_fixed + o_partial(), d_fixed + o_trace(), d_fixed + o_metric()}; }
    double* astat() const { return d_fixed + o_astat(); }
    void* tune() const { return d_fixed + o_tune(); }
};
namespace {
static_assert(LR_ADAPT_TRACE_COLS == lr::kAdaptTraceCols && lr::AD_SLOTS <= 8, "logreg_hip_adapt.h and lr_adapt.h");
static_assert(LR_ADAPT_WIDTH(3) == 4 && LR_ADAPT_WIDTH(8) == 8 && LR_ADAPT_WIDTH(9) == 16 && LR_ADAPT_WIDTH(20) == 32, "the fused kernels' padded widths");

// the schedule of include/logreg_hip_adapt.h; buffers already defaulted
int adapt_windows(int W, int init, int term, int base, int* ends, int* init_out) {
    int n = 0;
    if (W >= 20) {
        if ((int64_t)init + base + term > W) {
            init = (int)(0.15 * W);
            term = (int)(0.10 * W);
            base = W - init - term;
        }
        int64_t start = init, size = base;
        while (start < W - term && n < LR_ADAPT_MAX_WINDOWS && size > 0) {
            int64_t end = start + size;
            if (end + 2 * size > W - term) end = W - term;
            ends[n++] = (int)end;
            start = end;
            size *= 2;
        }
    }
    if (init_out) *init_out = n ? init : W;
    return n;
}

// the NutsTune block of (eps, dmm) a warm-up starts from
template <typename T, int P>
int tune_start(int p, double eps, const double* dmm, std::vector<unsigned char>* img) {
    lr::NutsTune<T, P> t{};
    diag_tuning(p, eps, dmm, &t.step, t.a, t.b, t.c);
    img->resize(sizeof(t));
    std::memcpy(img->data(), &t, sizeof(t));
    return LR_OK;
}
int tune_start_any(const lr_model* m, double eps, const double* dmm, std::vector<unsigned char>* img) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, m->dtype, m->P, tune_start, m->p, eps, dmm, img)
    return bad_width(m);
}

// What follows iteration h->t's NUTS launches on `st`: the pooled partials of `astat` [C] and of the states x [C][ld], the update of the tuning
// block, and the handle's count of where the schedule stands; the handle's dense part adds its co-moments inside a window and its window end.
template <typename T, int P>
int adapt_after(lr_adapt* h, hipStream_t st, const void* x, int64_t ld, const double* astat) {
    lr_model* m = h->m;
    DenseAdapt* dense = h->dense.get();
    const lr::AdaptDev dev = h->dev();
    const bool in_window = h->window < h->n_windows && h->t >= (h->window ? h->ends[h->window - 1] : h->init);
    const bool window_end = in_window && h->t == h->ends[h->window] - 1;
    const auto xs = static_cast<const T*>(x);
    if constexpr (P <= 32) hipLaunchKernelGGL((lr::k_adapt_partial<T, P>), dim3((unsigned)h->B), dim3(lr::kAdaptBlock), 0, st, xs, ld, astat, h->C, m->p, in_window ? 1 : 0, dev.partial);
    else hipLaunchKernelGGL((lr::k_tall_adapt_partial<T, P>), dim3((unsigned)h->B), dim3(lr::kAdaptBlock), 0, st, xs, ld, astat, h->C, m->p, in_window ? 1 : 0, dev.partial);
    LR_HIP(hipGetLastError());
    if constexpr (P <= 32) {  // (the dense metric: the fused kernels' widths, states [C][p])
        if (dense && in_window)
            if (const int rc = dense->accumulate<T, P>(st, const_cast<void*>(x), h->C, h->B, m->p)) return rc;
    }
    const lr::AdaptStep s{h->C, h->t, m->p, h->m_since + 1, in_window ? h->window : -1, window_end ? 1 : 0, h->t == h->W - 1 ? 1 : 0, h->delta, h->gamma, h->t0, h->kappa};
    auto* tune = static_cast<lr::NutsTune<T, P>*>(h->tune());
    if constexpr (P <= 32) hipLaunchKernelGGL((lr::k_adapt_update<T, P>), dim3(1), dim3(lr::adapt_update_lanes(P)), 0, st, dev, s, tune);
    else hipLaunchKernelGGL((lr::k_tall_adapt_update<T, P>), dim3(1), dim3(lr::adapt_update_lanes(P)), 0, st, dev, s, tune);
    LR_HIP(hipGetLastError());
    ++h->t;
    h->m_since = window_end ? 0 : h->m_since + 1;
    if (window_end) ++h->window;
    if (dense && window_end)
        if (const int rc = dense->window_end(m, st)) return rc;
    return LR_OK;
}

// `iters` iterations on `st`: the tuned NUTS launch, the pooled partials, the update; the handle's dense part adds its co-moments inside a
// window and its window end.  Every pointer is device memory; `o` has iters = thin = 1 and no statistics (lr_adapt_run).
template <typename T, int P>
int adapt_enqueue(lr_adapt* h, const Plan& pl, hipStream_t st, const lr_run_opts* o, int max_depth, void* state, void* out, lr_nuts_counters* counters,
                  int8_t* depth_out, double* astat_out, int64_t iters) {
    lr_model* m = h->m;
    DenseAdapt* dense = h->dense.get();
    auto* tune = static_cast<lr::NutsTune<T, P>*>(h->tune());
    const size_t row = (size_t)h->C * m->p;
    h->last = st;
    for (int64_t i = 0; i < iters; ++i) {
        lr_run_opts it = *o;
        it.iter_offset = LR_ADAPT_ITER_BASE + h->t;
        const NutsMetric mt{nullptr, dense ? dense->d_factor : nullptr, tune, astat_out ? astat_out + (size_t)i * h->C : h->astat(), "lr_adapt_run: "};
        const RunArrays d{state, nullptr, out ? static_cast<T*>(out) + (size_t)i * row : nullptr, counters, sizeof(lr_nuts_counters),
                          depth_out ? depth_out + (size_t)i * h->C : nullptr};
        if (const int rc = nuts_launch<T, P>(m, pl, st, &it, 0.0, max_depth, mt, d)) return rc;
        if (const int rc = adapt_after<T, P>(h, st, state, m->p, mt.astat)) return rc;
    }
    return LR_OK;
}
// ... and on the stepwise engine (include/logreg_hip_adapt_tall.h): ONE pass of the engine's NUTS loop over the call's iterations, the chains
// resident in its workspace, with adapt_after behind every iteration's end
template <typename T, int P>
int adapt_enqueue_tall(lr_adapt* h, const Plan& pl, hipStream_t st, const lr_run_opts* o, int max_depth, void* state, void* out, lr_nuts_counters* counters,
                       int8_t* depth_out, double* astat_out, int64_t iters) {
    h->last = st;
    lr_run_opts oo = *o;
    oo.iters = iters;
    oo.iter_offset = LR_ADAPT_ITER_BASE + h->t;
    RunSpec rs{};  // (the tuning is the handle's block)
    rs.kind = lr::KIND_HMC;
    const NutsWarm warm{h->tune(), [&](int64_t i) { return astat_out ? astat_out + (size_t)i * h->C : h->astat(); },
                        [&](int64_t, const void* x, int64_t ld, const double* astat) { return adapt_after<T, P>(h, st, x, ld, astat); }};
    return do_nuts_stepwise_t<T, P>(h->m, pl, st, rs, &oo, max_depth, state, out, counters, depth_out, &warm);
}
int adapt_enqueue_any(lr_adapt* h, const Plan& pl, hipStream_t st, const lr_run_opts* o, int max_depth, void* state, void* out, lr_nuts_counters* counters,
                      int8_t* depth_out, double* astat_out, int64_t iters) {
    if (h->tall) {
        LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, h->m->dtype, h->m->P, adapt_enqueue_tall, h, pl, st, o, max_depth, state, out, counters, depth_out, astat_out, iters)
        return bad_width(h->m);
    }
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, h->m->dtype, h->m->P, adapt_enqueue, h, pl, st, o, max_depth, state, out, counters, depth_out, astat_out, iters)
    return bad_width(h->m);
}
// ... and a failure of it ends the handle's use: an iteration may be enqueued without its update, so the tuning block and the trace no
// longer belong together (lr_adapt_run refuses the handle from then on; result and trace still read what is there)
int adapt_enqueue_checked(lr_adapt* h, const Plan& pl, hipStream_t st, const lr_run_opts* o, int max_depth, void* state, void* out, lr_nuts_counters* counters,
                          int8_t* depth_out, double* astat_out, int64_t iters) {
    const int rc = adapt_enqueue_any(h, pl, st, o, max_depth, state, out, counters, depth_out, astat_out, iters);
    // (the stepwise engine's workspace is allocated before anything is enqueued: out of memory there leaves the handle as it was)
    if (rc != LR_OK && !(h->tall && rc == LR_ERR_NOMEM)) h->failed = true;
    return rc;
}

// what lr_adapt_result and lr_dense_adapt_result report: the step size, the metric (`dense`: its Sigma and window counts, else the handle's dmm
// and the device's counts) and the counts
int adapt_result(lr_adapt* h, const DenseAdapt* dense, double* eps, double* metric, lr_adapt_info* info) {
    if (!h) return fail(LR_ERR_INVALID, "lr_adapt_result: handle is NULL");
    LR_HIP(hipSetDevice(h->m->device));
    LR_HIP(hipStreamSynchronize(h->last));
    double da[8];
    LR_HIP(hipMemcpy(da, h->d_fixed, sizeof(da), hipMemcpyDeviceToHost));
    if (eps) *eps = da[lr::AD_EPS_REPORT];
    if (metric && dense) std::copy(dense->sigma.begin(), dense->sigma.end(), metric);
    else if (metric) LR_HIP(hipMemcpy(metric, h->d_fixed + h->o_dmm(), (size_t)h->p() * sizeof(double), hipMemcpyDeviceToHost));
    if (info) *info = lr_adapt_info{h->t, dense ? dense->skipped : (int64_t)da[lr::AD_SKIPPED], dense ? dense->windows : (int32_t)da[lr::AD_WINDOWS], h->n_windows};
    return LR_OK;
}
// ... and the traces: [W][5], and the metric after each window (dmm: [windows][2][p] from the device; dense: [windows][p][p])
int adapt_trace(lr_adapt* h, const DenseAdapt* dense, double* trace, double* metric) {
    if (!h) return fail(LR_ERR_INVALID, "lr_adapt_trace: handle is NULL");
    LR_HIP(hipSetDevice(h->m->device));
    LR_HIP(hipStreamSynchronize(h->last));
    if (trace) LR_HIP(hipMemcpy(trace, h->d_fixed + h->o_trace(), (size_t)h->W * LR_ADAPT_TRACE_COLS * sizeof(double), hipMemcpyDeviceToHost));
    if (metric && dense) std::copy(dense->sigma_trace.begin(), dense->sigma_trace.end(), metric);
    else if (metric && h->n_windows > 0) LR_HIP(hipMemcpy(metric, h->d_fixed + h->o_metric(), (size_t)h->n_windows * 2 * h->p() * sizeof(double), hipMemcpyDeviceToHost));
    return LR_OK;
}
}  // namespace
extern "C" {

int lr_adapt_schedule(int32_t W, int32_t init_buffer, int32_t term_buffer, int32_t base_window, int32_t* ends, int32_t* n_windows, int32_t* init_out) {
    if (!ends || !n_windows) return fail(LR_ERR_INVALID, "lr_adapt_schedule: ends / n_windows is NULL");
    if (W < 1) return fail(LR_ERR_INVALID, "lr_adapt_schedule: W must be >= 1 (got %d)", W);
    if (init_buffer < 0 || term_buffer < 0 || base_window < 0)
        return fail(LR_ERR_INVALID, "lr_adapt_schedule: the buffers must be >= 0, 0 for the default (got %d, %d, %d)", init_buffer, term_buffer, base_window);
    *n_windows = adapt_windows(W, init_buffer ? init_buffer : 75, term_buffer ? term_buffer : 50, base_window ? base_window : 25, ends, init_out);
    return LR_OK;
}

namespace {
// lr_adapt_create and lr_tall_adapt_create (`tall`: on the stepwise engine, include/logreg_hip_adapt_tall.h): one set of argument checks, then
// the shapes each takes
int adapt_create(const char* who, bool tall, lr_model* m, int64_t C, const lr_adapt_opts* o, lr_adapt** out) {
    if (!m || !o || !out) return fail(LR_ERR_INVALID, "%s: model / opts / out is NULL", who);
    if (C <= 0) return fail(LR_ERR_INVALID, "%s: C must be positive (got %lld)", who, (long long)C);
    if (C > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "%s: %lld chains are beyond the launch grid", who, (long long)C);
    if (o->W < 1) return fail(LR_ERR_INVALID, "%s: W must be >= 1 (got %d)", who, o->W);
    if (o->init_buffer < 0 || o->term_buffer < 0 || o->base_window < 0)
        return fail(LR_ERR_INVALID, "%s: the buffers must be >= 0, 0 for the default (got %d, %d, %d)", who, o->init_buffer, o->term_buffer, o->base_window);
    if (!(o->delta >= 0 && o->delta < 1)) return fail(LR_ERR_INVALID, "%s: delta must be in (0, 1), 0 for the default 0.8 (got %g)", who, o->delta);
    if (!(o->eps0 >= 0) || !std::isfinite(o->eps0)) return fail(LR_ERR_INVALID, "%s: eps0 must be finite and > 0, 0 for the default 1 (got %g)", who, o->eps0);
    for (const double v : {o->gamma, o->t0, o->kappa})
        if (!(v >= 0) || !std::isfinite(v)) return fail(LR_ERR_INVALID, "%s: gamma, t0 and kappa must be finite and > 0, 0 for the defaults (got %g)", who, v);
    if (o->dmm0)
        if (const int rc = positive_vec((std::string(who) + ": dmm0").c_str(), o->dmm0, m->p)) return rc;
    if (!tall && (m->P > 32 || !m->table || !m->table->launch_nuts))
        return fail(LR_ERR_UNSUPPORTED, "NUTS: p = %d > 32 -- wide models run on the stepwise engine, which has no NUTS kernel", m->p);
    if (tall && nuts_fused_takes(m))
        return fail(LR_ERR_UNSUPPORTED, "%s: the stepwise (tall-data) engine takes the NUTS warm-up only where the fused kernel cannot (p > 32, or rows beyond the "
                    "LDS); here (n = %lld, p = %d) the warm-up is lr_adapt_create's, with the rows in LDS", who, (long long)m->n, m->p);
    if (tall && (!m->table || !m->table->launch_tall_nuts_tuned)) return fail(LR_ERR_UNSUPPORTED, "%s: no stepwise NUTS kernel for padded p = %d", who, m->P);
    if (const int rc = use_device(m->device, who)) return rc;
    std::unique_ptr<lr_adapt> h(new lr_adapt());
    h->m = m;
    h->tall = tall;
    h->C = C;
    h->B = (C + lr::kAdaptBlock - 1) / lr::kAdaptBlock;
    h->W = o->W;
    h->delta = o->delta > 0 ? o->delta : 0.8;
    h->gamma = o->gamma > 0 ? o->gamma : 0.05;
    h->t0 = o->t0 > 0 ? o->t0 : 10.0;
    h->kappa = o->kappa > 0 ? o->kappa : 0.75;
    h->n_windows = adapt_windows(o->W, o->init_buffer ? o->init_buffer : 75, o->term_buffer ? o->term_buffer : 50, o->base_window ? o->base_window : 25, h->ends, &h->init);
    if (!o->adapt_metric) h->n_windows = 0;
    const double eps0 = o->eps0 > 0 ? o->eps0 : 1.0;
    std::vector<double> dmm((size_t)m->p, 1.0);
    if (o->dmm0) std::copy(o->dmm0, o->dmm0 + m->p, dmm.begin());
    std::vector<unsigned char> tune;
    if (const int rc = tune_start_any(m, eps0, dmm.data(), &tune)) return rc;
    h->tune_bytes = tune.size();
    h->words = h->o_tune();
    const size_t want = h->words * sizeof(double) + h->tune_bytes;
    if (hipMalloc((void**)&h->d_fixed, want) != hipSuccess) return fail(LR_ERR_NOMEM, "%s: allocating %zu bytes of state failed", who, want);
    std::vector<double> img(h->words, 0.0);
    img[lr::AD_MU] = std::log(10.0 * eps0);
    img[lr::AD_EPS] = img[lr::AD_EPS_REPORT] = eps0;
    std::copy(dmm.begin(), dmm.end(), img.begin() + h->o_dmm());
    hipError_t e = hipMemcpy(h->d_fixed, img.data(), h->words * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->tune(), tune.data(), tune.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        lr_adapt_destroy(h.release());
        return fail(LR_ERR_HIP, "%s: copying the start state failed: %s", who, hipGetErrorString(e));
    }
    *out = h.release();
    return LR_OK;
}

// lr_adapt_run and lr_tall_adapt_run: one front; the handle says which engine runs the iterations, and the plan is that engine's
int adapt_run(const char* who, lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* o, void* out, lr_nuts_counters* counters, int8_t* depth_out,
              double* astat_out) {
    if (!h || !state || !o) return fail(LR_ERR_INVALID, "%s: handle / state / opts is NULL", who);
    if (h->failed) return fail(LR_ERR_HIP, "%s: a launch of an earlier call failed; this warm-up cannot go on (destroy the handle and start again)", who);
    if (iters < 0 || iters > h->W - h->t)
        return fail(LR_ERR_INVALID, "%s: iters must be in 0..%lld, the iterations that remain of W = %d (got %lld)", who, (long long)(h->W - h->t), h->W, (long long)iters);
    if (max_depth < 1 || max_depth > LR_NUTS_MAX_DEPTH) return fail(LR_ERR_INVALID, "%s: max_depth must be in 1..%d (got %d)", who, LR_NUTS_MAX_DEPTH, max_depth);
    if (o->n_chains != h->C) return fail(LR_ERR_INVALID, "%s: opts->n_chains must be the handle's %lld chains (got %lld)", who, (long long)h->C, (long long)o->n_chains);
    if (o->stats) return fail(LR_ERR_INVALID, "%s: opts->stats must be NULL (a warm-up keeps no streaming statistics)", who);
    lr_run_opts oo = *o;  // iters, thin and iter_offset are the warm-up's own (adapt_enqueue), the fields of the absent statistics as its launches have them
    oo.iters = 1;
    oo.thin = 1;
    oo.iter_offset = 0;
    oo.stats_batch = 1;
    oo.stats_first = 0;
    lr_model* m = h->m;
    if (const int rc = check_opts(m, &oo, true)) return rc;
    if (h->tall && oo.mode != LR_MODE_STEPWISE)
        return fail(LR_ERR_UNSUPPORTED, "%s: opts->mode must be LR_MODE_STEPWISE (got %d): the handle's iterations run on the stepwise engine", who, oo.mode);
    LR_HIP(hipSetDevice(m->device));
    Plan pl;
    if (const int rc = h->tall ? plan_nuts_stepwise(m, &oo, &pl) : plan_nuts(m, oo.group, oo.mode, max_depth, &pl, h->dense != nullptr)) return rc;
    if (iters == 0) return LR_OK;
    if (oo.on_device) return adapt_enqueue_checked(h, pl, (hipStream_t)oo.stream, &oo, max_depth, state, out, counters, depth_out, astat_out, iters);
    const size_t C = (size_t)h->C, sbytes = C * m->p * m->esize();
    struct { Workspace* ws; void* host; size_t bytes; bool in; const char* what; } const b[] = {
        {&h->st_state, state, sbytes, true, "staged state"},
        {&h->st_out, out, (size_t)iters * sbytes, false, "staged draws"},
        {&h->st_tally, counters, C * sizeof(lr_nuts_counters), true, "staged counters"},
        {&h->st_depth, depth_out, (size_t)iters * C, false, "staged depths"},
        {&h->st_astat, astat_out, (size_t)iters * C * sizeof(double), false, "staged acceptance statistics"}};
    for (const auto& q : b)
        if (q.host)
            if (const int rc = q.ws->grow(q.bytes, who, q.what)) return rc;
    for (const auto& q : b)
        if (q.host && q.in) LR_HIP(hipMemcpy(q.ws->p, q.host, q.bytes, hipMemcpyHostToDevice));
    auto dp = [&](int i) { return b[i].host ? b[i].ws->p : nullptr; };
    if (const int rc = adapt_enqueue_checked(h, pl, nullptr, &oo, max_depth, dp(0), dp(1), static_cast<lr_nuts_counters*>(dp(2)), static_cast<int8_t*>(dp(3)),
                                         static_cast<double*>(dp(4)), iters))
        return rc;
    LR_HIP(hipStreamSynchronize(nullptr));
    for (const auto& q : b)
        if (q.host) LR_HIP(hipMemcpy(q.host, q.ws->p, q.bytes, hipMemcpyDeviceToHost));
    return LR_OK;
}

}  // namespace

int lr_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* o, lr_adapt** out) { return adapt_create("lr_adapt_create", false, m, C, o, out); }

int lr_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* o, void* out, lr_nuts_counters* counters, int8_t* depth_out,
                 double* astat_out) {
    if (h && h->tall) return fail(LR_ERR_INVALID, "lr_adapt_run: the handle is one of lr_tall_adapt_create (lr_tall_adapt_run advances it)");
    return adapt_run("lr_adapt_run", h, state, iters, max_depth, o, out, counters, depth_out, astat_out);
}

// the warm-up on the stepwise engine (include/logreg_hip_adapt_tall.h): an lr_adapt whose iterations are the launches of lr_tall_nuts.h
int lr_tall_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* o, lr_adapt** out) { return adapt_create("lr_tall_adapt_create", true, m, C, o, out); }

int lr_tall_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* o, void* out, lr_nuts_counters* counters, int8_t* depth_out,
                      double* astat_out) {
    if (h && !h->tall) return fail(LR_ERR_INVALID, "lr_tall_adapt_run: the handle is not one of lr_tall_adapt_create");
    return adapt_run("lr_tall_adapt_run", h, state, iters, max_depth, o, out, counters, depth_out, astat_out);
}

int lr_adapt_result(lr_adapt* h, double* eps, double* dmm, lr_adapt_info* info) { return adapt_result(h, nullptr, eps, dmm, info); }

int lr_adapt_trace(lr_adapt* h, double* trace, double* metric) { return adapt_trace(h, nullptr, trace, metric); }

void lr_adapt_destroy(lr_adapt* h) {
    if (!h) return;
    (void)hipSetDevice(h->m->device);
    free_all({h->d_fixed, h->st_state.p, h->st_out.p, h->st_tally.p, h->st_depth.p, h->st_astat.p});
    delete h;  // (and with it the dense part and its two buffers)
}

// the warm-up under a dense metric (include/logreg_hip_dense.h): an lr_adapt whose iterations run k_nuts_dense and whose windows, with
// adapt_metric, re-estimate the full inverse metric
int lr_dense_adapt_create(lr_model* m, int64_t C, const lr_adapt_opts* o, const double* inv_metric, lr_adapt** out) {
    if (!m || !o || !out) return fail(LR_ERR_INVALID, "lr_dense_adapt_create: model / opts / out is NULL");
    if (o->dmm0) return fail(LR_ERR_INVALID, "lr_dense_adapt_create: dmm0 must be NULL (the metric is inv_metric)");
    if (m->P > 32) return fail(LR_ERR_UNSUPPORTED, "NUTS: p = %d > 32 -- wide models run on the stepwise engine, which has no NUTS kernel", m->p);
    const int p = m->p;
    std::vector<double> sigma((size_t)p * p, 0.0);
    if (inv_metric) {
        for (int i = 0; i < p; ++i)
            for (int j = 0; j <= i; ++j) sigma[(size_t)i * p + j] = sigma[(size_t)j * p + i] = inv_metric[(size_t)i * p + j];
    } else {
        for (int i = 0; i < p; ++i) sigma[(size_t)i * p + i] = 1.0;  // NULL: the unit metric
    }
    DenseFactorHost f;
    if (const int rc = dense_factor_host(m, "lr_dense_adapt_create", sigma.data(), &f)) return rc;
    if (!m->table || !m->table->launch_nuts) return fail(LR_ERR_UNSUPPORTED, "NUTS: no kernel for padded p = %d", m->P);
    lr_adapt* h = nullptr;
    if (const int rc = lr_adapt_create(m, C, o, &h)) return rc;
    h->dense.reset(new DenseAdapt());
    DenseAdapt* d = h->dense.get();
    d->sigma = sigma;
    d->sigma_trace.assign((size_t)h->n_windows * p * p, 0.0);
    const size_t cm_bytes = (size_t)(h->B + 1) * lr::dense_triple_words(m->P) * sizeof(double);
    hipError_t e = hipMalloc(&d->d_factor, f.image.size());
    if (e != hipSuccess) d->d_factor = nullptr;
    if (e == hipSuccess && h->n_windows > 0) {  // adapt_metric: the windows re-estimate Sigma
        e = hipMalloc((void**)&d->d_comoment, cm_bytes);
        if (e != hipSuccess) d->d_comoment = nullptr;
    }
    if (e != hipSuccess) {
        lr_adapt_destroy(h);
        return fail(LR_ERR_NOMEM, "lr_dense_adapt_create: allocating the metric's factor and co-moments failed");
    }
    e = hipMemcpy(d->d_factor, f.image.data(), f.image.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && d->d_comoment) {  // an empty window
        const std::vector<double> zero((size_t)lr::dense_triple_words(m->P), 0.0);
        e = hipMemcpy(d->d_comoment, zero.data(), zero.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        lr_adapt_destroy(h);
        return fail(LR_ERR_HIP, "lr_dense_adapt_create: copying the metric's factor failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return LR_OK;
}
int lr_dense_adapt_run(lr_adapt* h, void* state, int64_t iters, int32_t max_depth, const lr_run_opts* o, void* out, lr_nuts_counters* counters,
                       int8_t* depth_out, double* astat_out) {
    if (h && !h->dense) return fail(LR_ERR_INVALID, "lr_dense_adapt_run: the handle is not one of lr_dense_adapt_create");
    return lr_adapt_run(h, state, iters, max_depth, o, out, counters, depth_out, astat_out);
}
int lr_dense_adapt_result(lr_adapt* h, double* eps, double* inv_metric, lr_adapt_info* info) {
    if (h && !h->dense) return fail(LR_ERR_INVALID, "lr_dense_adapt_result: the handle is not one of lr_dense_adapt_create");
    return adapt_result(h, h ? h->dense.get() : nullptr, eps, inv_metric, info);
}
int lr_dense_adapt_trace(lr_adapt* h, double* trace, double* metric) {
    if (h && !h->dense) return fail(LR_ERR_INVALID, "lr_dense_adapt_trace: the handle is not one of lr_dense_adapt_create");
    return adapt_trace(h, h ? h->dense.get() : nullptr, trace, metric);
}
void lr_dense_adapt_destroy(lr_adapt* h) { lr_adapt_destroy(h); }

// ---- PSIS-LOO: the pointwise log-likelihood matrix and its Pareto-smoothed leave-one-out summary (include/logreg_hip_loo.h; kernels: lr_loo.h)
}  // extern "C"
struct lr_loo : Staged {
    lr_model* m = nullptr;
    int device = 0;              // the model's (kept here: lr_loo_destroy must not need the model)
    int64_t n = 0;               // the model's rows
    int64_t cap = 0, ld = 0;     // max_draws; the row stride of the matrix (cap rounded up to 128 bytes)
    size_t es = 0;               // bytes per value: the model's dtype
    int32_t dtype = LR_F32;
    void* d_ll = nullptr;        // [n][ld]
    double* d_table = nullptr;   // [LR_LOO_ROWS][n]
    int64_t S = 0;               // draws held
    Workspace out;               // the matrix transposed for lr_loo_loglik
};
namespace {
static_assert(LR_LOO_ROWS == lr::kLooRows && LR_LOO_MAX_DRAWS == lr::kLooMaxDraws, "logreg_hip_loo.h and lr_loo.h");

template <typename T, int P>
int loo_fill(lr_loo* a, const void* d_draws, int64_t S, hipStream_t st) {
    constexpr int64_t TS = lr::kLooTileBytes / (int)sizeof(T);
    const int64_t tiles = (a->n + lr::kLooBlock - 1) / lr::kLooBlock;
    const int64_t want_blocks = (int64_t)(a->m->cus > 0 ? a->m->cus : 256) * 4;  // four waves on every SIMD, at least 64 draws a slice
    const int64_t sl = std::max<int64_t>(1, (want_blocks + tiles - 1) / tiles);
    int64_t per = std::max<int64_t>(64, (S + sl - 1) / sl);
    per = (per + TS - 1) / TS * TS;
    const int64_t slices = (S + per - 1) / per;
    hipLaunchKernelGGL((lr::k_loo_fill<T, P>), dim3((unsigned)tiles, (unsigned)slices), dim3(lr::kLooBlock), 0, st, static_cast<const T*>(a->m->d_rows), a->n,
                       static_cast<const T*>(d_draws), S, per, static_cast<T*>(a->d_ll), a->ld, a->S);
    LR_HIP(hipGetLastError());
    a->S += S;
    return LR_OK;
}
int loo_fill_any(lr_loo* a, const void* d_draws, int64_t S, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, a->m->dtype, a->m->P, loo_fill, a, d_draws, S, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_loo: unsupported padded width %d", a->m->P);
}

// src [A][lds] -> dst [B][ldd] on the device
template <typename T>
int loo_transpose(const void* src, int64_t A, int64_t B, int64_t lds, void* dst, int64_t ldd, hipStream_t st) {
    hipLaunchKernelGGL(lr::k_loo_transpose<T>, dim3((unsigned)((A + 31) / 32), (unsigned)((B + 31) / 32)), dim3(32, 8), 0, st, static_cast<const T*>(src), A, B, lds,
                       static_cast<T*>(dst), ldd);
    LR_HIP(hipGetLastError());
    return LR_OK;
}

// the PSIS stage over d_ll [r][ld] (S draws a row) -> d_table [LR_LOO_ROWS][r]; 0 < S <= LR_LOO_MAX_DRAWS
template <typename T>
int loo_psis(const void* d_ll, int64_t ld, int64_t S, int64_t r, double* d_table, hipStream_t st) {
    const int M = (int)lr::loo_tail_len(S);
    if (S <= lr::kLooSmallDraws)
        hipLaunchKernelGGL((lr::k_psis<T, 256, 1024, 1024>), dim3((unsigned)r), dim3(256), 0, st, static_cast<const T*>(d_ll), ld, (int)S, M, r, d_table);
    else
        hipLaunchKernelGGL((lr::k_psis<T, 512, 4096, 3072>), dim3((unsigned)r), dim3(512), 0, st, static_cast<const T*>(d_ll), ld, (int)S, M, r, d_table);
    LR_HIP(hipGetLastError());
    return LR_OK;
}
}  // namespace
extern "C" {

int lr_loo_create(lr_model* m, int64_t max_draws, lr_loo** out) {
    if (!m || !out) return fail(LR_ERR_INVALID, "lr_loo_create: model / out is NULL");
    if (max_draws <= 0) return fail(LR_ERR_INVALID, "lr_loo_create: max_draws must be positive (got %lld)", (long long)max_draws);
    if (max_draws > LR_LOO_MAX_DRAWS)
        return fail(LR_ERR_UNSUPPORTED, "lr_loo_create: max_draws = %lld is beyond LR_LOO_MAX_DRAWS = %d (the tail of an observation is sorted in on-chip memory)",
                    (long long)max_draws, LR_LOO_MAX_DRAWS);
    if (m->n > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "lr_loo_create: n = %lld is beyond the launch grid", (long long)m->n);
    LR_HIP(hipSetDevice(m->device));
    lr_loo* a = new lr_loo();
    a->m = m;
    a->device = m->device;
    a->n = m->n;
    a->dtype = m->dtype;
    a->es = m->esize();
    a->cap = max_draws;
    const int64_t line = lr::kLooTileBytes / (int64_t)a->es;
    a->ld = (max_draws + line - 1) / line * line;
    const size_t want = (size_t)a->n * a->ld * a->es;
    if (hipMalloc(&a->d_ll, want) != hipSuccess) {
        lr_loo_destroy(a);
        return fail(LR_ERR_NOMEM, "lr_loo_create: allocating %zu bytes for the log-likelihood of %lld rows x %lld draws failed", want, (long long)m->n, (long long)max_draws);
    }
    if (hipMalloc((void**)&a->d_table, (size_t)LR_LOO_ROWS * a->n * sizeof(double)) != hipSuccess) {
        lr_loo_destroy(a);
        return fail(LR_ERR_NOMEM, "lr_loo_create: allocating the table failed");
    }
    *out = a;
    return LR_OK;
}

int lr_loo_accumulate(lr_loo* a, const void* draws, int64_t S, int32_t on_device, void* stream) {
    if (!a || !draws) return fail(LR_ERR_INVALID, "lr_loo_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_loo_accumulate: S must be positive (got %lld)", (long long)S);
    if (S > a->cap - a->S)
        return fail(LR_ERR_INVALID, "lr_loo_accumulate: %lld draws held + %lld more exceed max_draws = %lld", (long long)a->S, (long long)S, (long long)a->cap);
    LR_HIP(hipSetDevice(a->device));
    return stage_draws(
        "lr_loo", *a, a->m, Feed{draws, S, on_device != 0, (hipStream_t)stream}, [](int64_t) { return LR_OK; },
        [a](const void* d_draws, int64_t Sb, hipStream_t st) { return loo_fill_any(a, d_draws, Sb, st); });
}

int lr_loo_loglik(lr_loo* a, void* host_out, int64_t* n_draws) {
    if (!a) return fail(LR_ERR_INVALID, "lr_loo_loglik: accumulator is NULL");
    if (n_draws) *n_draws = a->S;
    if (!host_out || a->S == 0) return LR_OK;
    LR_HIP(hipSetDevice(a->device));
    const size_t bytes = (size_t)a->S * a->n * a->es;
    if (const int rc = a->out.grow(bytes, "lr_loo", "the transposed matrix")) return rc;
    if (const int rc = LR_BY_DTYPE(a->dtype, loo_transpose, a->d_ll, a->n, a->S, a->ld, a->out.p, a->n, a->last)) return rc;
    LR_HIP(hipMemcpyAsync(host_out, a->out.p, bytes, hipMemcpyDeviceToHost, a->last));
    LR_HIP(hipStreamSynchronize(a->last));
    return LR_OK;
}

int lr_loo_result(lr_loo* a, double* table, int64_t* n_draws) {
    if (!a || !table) return fail(LR_ERR_INVALID, "lr_loo_result: accumulator / table is NULL");
    if (n_draws) *n_draws = a->S;
    const size_t cells = (size_t)LR_LOO_ROWS * a->n;
    if (a->S == 0) {
        fill_nan(table, cells);
        return LR_OK;
    }
    LR_HIP(hipSetDevice(a->device));
    if (const int rc = LR_BY_DTYPE(a->dtype, loo_psis, a->d_ll, a->ld, a->S, a->n, a->d_table, a->last)) return rc;
    LR_HIP(hipMemcpyAsync(table, a->d_table, cells * sizeof(double), hipMemcpyDeviceToHost, a->last));
    LR_HIP(hipStreamSynchronize(a->last));
    return LR_OK;
}

int lr_loo_reset(lr_loo* a) {
    if (!a) return fail(LR_ERR_INVALID, "lr_loo_reset: accumulator is NULL");
    a->S = 0;  // the next draws overwrite the matrix from its first column
    return LR_OK;
}

void lr_loo_destroy(lr_loo* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    free_all({a->d_ll, a->d_table, a->in.p, a->padded.p, a->out.p});
    delete a;
}

int lr_psis(int device, const void* loglik, int64_t S, int64_t r, int32_t dtype, int32_t on_device, double* table, void* stream) {
    if (!loglik || !table) return fail(LR_ERR_INVALID, "lr_psis: loglik / table is NULL");
    if (S <= 0 || r <= 0) return fail(LR_ERR_INVALID, "lr_psis: S and r must be positive (got %lld, %lld)", (long long)S, (long long)r);
    if (dtype != LR_F32 && dtype != LR_F64) return fail(LR_ERR_INVALID, "lr_psis: dtype must be LR_F32 or LR_F64");
    if (S > LR_LOO_MAX_DRAWS)
        return fail(LR_ERR_UNSUPPORTED, "lr_psis: S = %lld is beyond LR_LOO_MAX_DRAWS = %d (the tail of an observation is sorted in on-chip memory)", (long long)S,
                    LR_LOO_MAX_DRAWS);
    if (r > 65535ll * 32) return fail(LR_ERR_UNSUPPORTED, "lr_psis: r = %lld is beyond the launch grid", (long long)r);
    if (const int rc = use_device(device, "lr_psis", true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t es = dtype == LR_F32 ? 4 : 8;
    const int64_t line = lr::kLooTileBytes / (int64_t)es, ld = (S + line - 1) / line * line;
    DevBuf din, dt, dtab;
    if ((!on_device && din.alloc((size_t)S * r * es)) || dt.alloc((size_t)r * ld * es) || dtab.alloc((size_t)LR_LOO_ROWS * r * sizeof(double)))
        return fail(LR_ERR_NOMEM, "lr_psis: allocating the workspaces of a %lld x %lld matrix failed", (long long)S, (long long)r);
    const void* src = loglik;
    if (!on_device) {
        LR_HIP(hipMemcpyAsync(din.p, loglik, (size_t)S * r * es, hipMemcpyHostToDevice, st));
        src = din.p;
    }
    int rc = LR_BY_DTYPE(dtype, loo_transpose, src, S, r, r, dt.p, ld, st);
    if (!rc) rc = LR_BY_DTYPE(dtype, loo_psis, dt.p, ld, S, r, static_cast<double*>(dtab.p), st);
    if (rc) {
        (void)hipStreamSynchronize(st);  // the workspaces are freed on return
        return rc;
    }
    LR_HIP(hipMemcpyAsync(table, dtab.p, (size_t)LR_LOO_ROWS * r * sizeof(double), hipMemcpyDeviceToHost, st));
    LR_HIP(hipStreamSynchronize(st));
    return LR_OK;
}

// ---- bridge sampling: the log marginal likelihood from the draws (include/logreg_hip_bridge.h; kernels: lr_bridge.h) -------------------
}  // extern "C"
struct lr_bridge : Staged {
    lr_model* m = nullptr;
    int device = 0;               // the model's (kept here: lr_bridge_destroy must not need the model)
    int64_t cap = 0, N1 = 0, N2 = 0;
    uint64_t seed = 0;
    double cg = 0;                // -sum log L_ii - p / 2 log(2 pi)
    double* d_prop = nullptr;     // mu [p] | inv_var [p] | W packed | L packed
    double* d_l1 = nullptr;       // [cap]
    double* d_l2 = nullptr;       // [N2]
    double* d_iter = nullptr;     // the partials of a pass [blocks][3], then the state [BS_SLOTS]
    Workspace part;               // row-slice partials of one chunk of draws
    Workspace prop;               // a chunk of proposal draws [chunk][P]
};
namespace {
static_assert(LR_BRIDGE_ROWS == lr::kBridgeRows && LR_BRIDGE_MAX_DRAWS == lr::kBridgeMaxDraws && LR_BRIDGE_TAG == lr::TAG_BRIDGE, "logreg_hip_bridge.h and lr_bridge.h");

constexpr int64_t kBridgePropChunk = 1 << 16;  // proposal draws generated at a time
int64_t bridge_blocks(int64_t N) { return (N + lr::kBridgeChunk - 1) / lr::kBridgeChunk; }
int64_t bridge_row_slices(int64_t n) { return (n + lr::kBridgeSliceRows - 1) / lr::kBridgeSliceRows; }
// draws whose row-slice partials are held at a time: 64 MB of them, at least 1024 draws
int64_t bridge_chunk(int64_t n) { return std::max<int64_t>(1024, (int64_t)((size_t(64) << 20) / ((size_t)bridge_row_slices(n) * sizeof(double)))); }
int bridge_reserve(lr_bridge* a, int64_t S) {
    return a->part.grow((size_t)bridge_row_slices(a->m->n) * std::min(S, bridge_chunk(a->m->n)) * sizeof(double), "lr_bridge", "row-slice partials");
}

// the terms of S device-resident draws [S][P] -> d_out [S]; a->part holds a chunk (bridge_reserve)
template <typename T, int P>
int bridge_terms(lr_bridge* a, const void* d_draws, int64_t S, double* d_out, hipStream_t st) {
    const lr_model* m = a->m;
    const int64_t rsl = bridge_row_slices(m->n), chunk = bridge_chunk(m->n);
    const int64_t want_blocks = (int64_t)(m->cus > 0 ? m->cus : 256) * 4;  // four waves on every SIMD, at least 64 draws a slice
    for (int64_t c0 = 0; c0 < S; c0 += chunk) {
        const int64_t cs = std::min(chunk, S - c0);
        const int64_t sl = std::max<int64_t>(1, (want_blocks + rsl - 1) / rsl);
        const int64_t per = std::max<int64_t>(64, (cs + sl - 1) / sl), dsl = (cs + per - 1) / per;
        const T* d = static_cast<const T*>(d_draws) + c0 * P;
        hipLaunchKernelGGL((lr::k_bridge_fill<T, P>), dim3((unsigned)rsl, (unsigned)dsl), dim3(lr::kBridgeBlock), 0, st, static_cast<const T*>(m->d_rows), m->n, d, cs,
                           per, static_cast<double*>(a->part.p), cs);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL((lr::k_bridge_gauss<T, P>), dim3((unsigned)((cs + lr::kBridgeGaussBlock - 1) / lr::kBridgeGaussBlock)), dim3(lr::kBridgeGaussBlock), 0, st,
                           d, cs, m->p, static_cast<const double*>(a->part.p), cs, rsl, static_cast<const double*>(a->d_prop), a->cg, m->lprior_const, d_out + c0);
        LR_HIP(hipGetLastError());
    }
    return LR_OK;
}
int bridge_terms_any(lr_bridge* a, const void* d_draws, int64_t S, double* d_out, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, a->m->dtype, a->m->P, bridge_terms, a, d_draws, S, d_out, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_bridge: unsupported padded width %d", a->m->P);
}

// proposal draws [j0, j0 + cnt) -> a->prop [cnt][ldo], ldo = P or p
template <typename T, int P>
int bridge_propose(lr_bridge* a, int64_t j0, int64_t cnt, int ldo, hipStream_t st) {
    hipLaunchKernelGGL((lr::k_bridge_propose<T, P>), dim3((unsigned)((cnt + lr::kBridgeGaussBlock - 1) / lr::kBridgeGaussBlock)), dim3(lr::kBridgeGaussBlock), 0, st,
                       a->seed, j0, cnt, a->m->p, ldo, static_cast<const double*>(a->d_prop), static_cast<T*>(a->prop.p));
    LR_HIP(hipGetLastError());
    return LR_OK;
}
int bridge_propose_any(lr_bridge* a, int64_t j0, int64_t cnt, int ldo, hipStream_t st) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, a->m->dtype, a->m->P, bridge_propose, a, j0, cnt, ldo, st)
    return fail(LR_ERR_UNSUPPORTED, "lr_bridge: unsupported padded width %d", a->m->P);
}

// The iteration and the error over device-resident terms -> table (host).  d_iter: 3 (blocks of N1 + blocks of N2) + BS_SLOTS doubles.
// The host loops: it reads (log r, the previous log r) after every pass (lr_bridge.h says why).
int bridge_solve(const double* d_l1, int64_t N1, const double* d_l2, int64_t N2, double n_eff, double tol, int maxit, double* d_iter, hipStream_t st,
                 double* table) {
    const int64_t nb1 = bridge_blocks(N1), nb2 = bridge_blocks(N2);
    double* d_st = d_iter + 3 * (nb1 + nb2);
    const double n1 = (double)N1, n2 = (double)N2, neff = n_eff > 0 && std::isfinite(n_eff) ? n_eff : n1;
    const double s1 = neff / (neff + n2), s2 = n2 / (neff + n2), ls1 = std::log(s1), ls2 = std::log(s2);
    const auto pass = [&](int mode) {
        const int64_t blocks = mode == lr::BR_INIT ? nb2 : nb1 + nb2;
        hipLaunchKernelGGL(lr::k_bridge_iterate, dim3((unsigned)blocks), dim3(lr::kBridgeBlock), 0, st, mode, d_l1, N1, d_l2, N2, nb2, ls1, ls2, s1, s2,
                           static_cast<const double*>(d_st), d_iter);
        LR_HIP(hipGetLastError());
        hipLaunchKernelGGL(lr::k_bridge_finish, dim3(1), dim3(lr::kBridgeBlock), 0, st, mode, static_cast<const double*>(d_iter), nb1, nb2, n1, n2, neff, ls1, ls2,
                           s1, s2, d_st);
        LR_HIP(hipGetLastError());
        return (int)LR_OK;
    };
    double h[lr::BS_SLOTS];
    const auto read = [&](int count) {
        LR_HIP(hipMemcpyAsync(h, d_st, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
        LR_HIP(hipStreamSynchronize(st));
        return (int)LR_OK;
    };
    fill_nan(table, LR_BRIDGE_ROWS);
    if (const int rc = pass(lr::BR_SCAN)) return rc;
    if (const int rc = read(lr::BS_SLOTS)) return rc;
    table[2] = 0.0;
    table[3] = 0.0;
    table[4] = n1;
    table[5] = n2;
    table[6] = neff;
    table[7] = h[lr::BS_BAD];
    table[8] = h[lr::BS_MIN1];
    table[9] = h[lr::BS_MAX1];
    table[10] = h[lr::BS_MIN2];
    table[11] = h[lr::BS_MAX2];
    if (h[lr::BS_BAD] != 0.0) return LR_OK;  // a term that is not finite: logml and se stay NaN
    if (const int rc = pass(lr::BR_INIT)) return rc;
    int it = 0, conv = 0;
    while (it < maxit && !conv) {
        if (const int rc = pass(lr::BR_ITER)) return rc;
        if (const int rc = read(2)) return rc;
        ++it;
        const double mag = std::fabs(h[lr::BS_LOGR]);
        conv = std::fabs(h[lr::BS_LOGR] - h[lr::BS_PREV]) <= tol * (mag > 1.0 ? mag : 1.0);
    }
    if (const int rc = pass(lr::BR_ERR)) return rc;
    if (const int rc = read(lr::BS_SLOTS)) return rc;
    table[0] = h[lr::BS_LOGR];
    table[1] = std::sqrt(h[lr::BS_RE2]);
    table[2] = (double)it;
    table[3] = (double)conv;
    return LR_OK;
}
int bridge_check_solve(const char* who, double tol, int maxit) {
    if (!(tol >= 0.0)) return fail(LR_ERR_INVALID, "%s: tol must be >= 0 (got %g)", who, tol);
    if (maxit < 0) return fail(LR_ERR_INVALID, "%s: maxit must be >= 0 (got %d)", who, maxit);
    return LR_OK;
}
}  // namespace
extern "C" {

int lr_bridge_create(lr_model* m, const double* mu, const double* cov, int64_t max_draws, int64_t n_proposal, uint64_t seed, lr_bridge** out) {
    if (!m || !mu || !cov || !out) return fail(LR_ERR_INVALID, "lr_bridge_create: model / mu / cov / out is NULL");
    if (max_draws <= 0 || n_proposal <= 0)
        return fail(LR_ERR_INVALID, "lr_bridge_create: max_draws and n_proposal must be positive (got %lld, %lld)", (long long)max_draws, (long long)n_proposal);
    if (max_draws > LR_BRIDGE_MAX_DRAWS || n_proposal > LR_BRIDGE_MAX_DRAWS)
        return fail(LR_ERR_UNSUPPORTED, "lr_bridge_create: max_draws = %lld / n_proposal = %lld is beyond LR_BRIDGE_MAX_DRAWS = %d", (long long)max_draws,
                    (long long)n_proposal, LR_BRIDGE_MAX_DRAWS);
    if (bridge_row_slices(m->n) > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "lr_bridge_create: n = %lld is beyond the launch grid", (long long)m->n);
    const int p = m->p;
    const size_t tri = (size_t)p * (p + 1) / 2;
    std::vector<double> host(2 * (size_t)p + 2 * tri);
    double cg = 0;
    char why[160];
    if (lr::bridge_factor(p, mu, cov, host.data() + 2 * p + tri, host.data() + 2 * p, &cg, why, sizeof(why))) return fail(LR_ERR_INVALID, "lr_bridge_create: %s", why);
    std::copy(mu, mu + p, host.begin());
    std::copy(m->inv_var, m->inv_var + p, host.begin() + p);
    LR_HIP(hipSetDevice(m->device));
    lr_bridge* a = new lr_bridge();
    a->m = m;
    a->device = m->device;
    a->cap = max_draws;
    a->N2 = n_proposal;
    a->seed = seed;
    a->cg = cg;
    const int64_t pc = std::min(n_proposal, kBridgePropChunk);
    const size_t iter_doubles = 3 * (size_t)(bridge_blocks(max_draws) + bridge_blocks(n_proposal)) + lr::BS_SLOTS;
    int rc = upload("lr_bridge_create", "proposal", host.data(), host.size() * sizeof(double), (void**)&a->d_prop, LR_ERR_HIP);
    if (!rc && (hipMalloc((void**)&a->d_l1, (size_t)max_draws * sizeof(double)) != hipSuccess || hipMalloc((void**)&a->d_l2, (size_t)n_proposal * sizeof(double)) != hipSuccess ||
                hipMalloc((void**)&a->d_iter, iter_doubles * sizeof(double)) != hipSuccess))
        rc = fail(LR_ERR_NOMEM, "lr_bridge_create: allocating the terms of %lld + %lld draws failed", (long long)max_draws, (long long)n_proposal);
    if (!rc) rc = a->prop.grow((size_t)pc * m->P * m->esize(), "lr_bridge_create", "proposal draws");
    if (!rc) rc = bridge_reserve(a, pc);
    for (int64_t j0 = 0; !rc && j0 < n_proposal; j0 += pc) {  // the proposal terms, on the NULL stream
        const int64_t cnt = std::min(pc, n_proposal - j0);
        rc = bridge_propose_any(a, j0, cnt, m->P, nullptr);
        if (!rc) rc = bridge_terms_any(a, a->prop.p, cnt, a->d_l2 + j0, nullptr);
    }
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(LR_ERR_HIP, "lr_bridge_create: computing the proposal terms failed");
    if (rc) {
        lr_bridge_destroy(a);
        return rc;
    }
    *out = a;
    return LR_OK;
}

int lr_bridge_accumulate(lr_bridge* a, const void* draws, int64_t S, int32_t on_device, void* stream) {
    if (!a || !draws) return fail(LR_ERR_INVALID, "lr_bridge_accumulate: accumulator / draws is NULL");
    if (S <= 0) return fail(LR_ERR_INVALID, "lr_bridge_accumulate: S must be positive (got %lld)", (long long)S);
    if (S > a->cap - a->N1)
        return fail(LR_ERR_INVALID, "lr_bridge_accumulate: %lld draws held + %lld more exceed max_draws = %lld", (long long)a->N1, (long long)S, (long long)a->cap);
    LR_HIP(hipSetDevice(a->device));
    return stage_draws(
        "lr_bridge", *a, a->m, Feed{draws, S, on_device != 0, (hipStream_t)stream}, [a](int64_t S0) { return bridge_reserve(a, S0); },
        [a](const void* d_draws, int64_t Sb, hipStream_t st) {
            if (const int rc = bridge_terms_any(a, d_draws, Sb, a->d_l1 + a->N1, st)) return rc;
            a->N1 += Sb;
            return (int)LR_OK;
        });
}

int lr_bridge_terms(lr_bridge* a, double* l1, double* l2, int64_t* n1, int64_t* n2) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_terms: accumulator is NULL");
    if (n1) *n1 = a->N1;
    if (n2) *n2 = a->N2;
    LR_HIP(hipSetDevice(a->device));
    if (l1 && a->N1 > 0) LR_HIP(hipMemcpyAsync(l1, a->d_l1, (size_t)a->N1 * sizeof(double), hipMemcpyDeviceToHost, a->last));
    if (l2) LR_HIP(hipMemcpyAsync(l2, a->d_l2, (size_t)a->N2 * sizeof(double), hipMemcpyDeviceToHost, a->last));
    LR_HIP(hipStreamSynchronize(a->last));
    return LR_OK;
}

int lr_bridge_proposal(lr_bridge* a, void* host_out, int64_t* n2) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_proposal: accumulator is NULL");
    if (n2) *n2 = a->N2;
    if (!host_out) return LR_OK;
    LR_HIP(hipSetDevice(a->device));
    const lr_model* m = a->m;
    const int64_t pc = std::min(a->N2, kBridgePropChunk);
    const size_t es = m->esize();
    LR_HIP(hipStreamSynchronize(a->last));  // a->prop is about to be overwritten
    for (int64_t j0 = 0; j0 < a->N2; j0 += pc) {
        const int64_t cnt = std::min(pc, a->N2 - j0);
        if (const int rc = bridge_propose_any(a, j0, cnt, m->p, a->last)) return rc;
        LR_HIP(hipMemcpyAsync(static_cast<unsigned char*>(host_out) + (size_t)j0 * m->p * es, a->prop.p, (size_t)cnt * m->p * es, hipMemcpyDeviceToHost, a->last));
        LR_HIP(hipStreamSynchronize(a->last));
    }
    return LR_OK;
}

int lr_bridge_result(lr_bridge* a, double n_eff, double tol, int32_t maxit, double* table) {
    if (!a || !table) return fail(LR_ERR_INVALID, "lr_bridge_result: accumulator / table is NULL");
    if (const int rc = bridge_check_solve("lr_bridge_result", tol, maxit)) return rc;
    if (a->N1 == 0) {
        fill_nan(table, LR_BRIDGE_ROWS);
        table[2] = table[3] = table[4] = 0.0;
        table[5] = (double)a->N2;
        return LR_OK;
    }
    LR_HIP(hipSetDevice(a->device));
    return bridge_solve(a->d_l1, a->N1, a->d_l2, a->N2, n_eff, tol, maxit, a->d_iter, a->last, table);
}

int lr_bridge_reset(lr_bridge* a) {
    if (!a) return fail(LR_ERR_INVALID, "lr_bridge_reset: accumulator is NULL");
    a->N1 = 0;  // the next draws overwrite the posterior terms from the first; the proposal terms stay
    return LR_OK;
}

void lr_bridge_destroy(lr_bridge* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    free_all({a->d_prop, a->d_l1, a->d_l2, a->d_iter, a->part.p, a->prop.p, a->in.p, a->padded.p});
    delete a;
}

int lr_bridge_solve(int device, const double* l1, int64_t N1, const double* l2, int64_t N2, double n_eff, double tol, int32_t maxit, int32_t on_device,
                    double* table, void* stream) {
    if (!l1 || !l2 || !table) return fail(LR_ERR_INVALID, "lr_bridge_solve: l1 / l2 / table is NULL");
    if (N1 <= 0 || N2 <= 0) return fail(LR_ERR_INVALID, "lr_bridge_solve: N1 and N2 must be positive (got %lld, %lld)", (long long)N1, (long long)N2);
    if (const int rc = bridge_check_solve("lr_bridge_solve", tol, maxit)) return rc;
    if (N1 > 0x7FFFFFFFll || N2 > 0x7FFFFFFFll) return fail(LR_ERR_UNSUPPORTED, "lr_bridge_solve: N1 = %lld / N2 = %lld is beyond 2^31 - 1", (long long)N1, (long long)N2);
    if (const int rc = use_device(device, "lr_bridge_solve", true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf d1, d2, dit;
    if ((!on_device && (d1.alloc((size_t)N1 * sizeof(double)) || d2.alloc((size_t)N2 * sizeof(double)))) ||
        dit.alloc((3 * (size_t)(bridge_blocks(N1) + bridge_blocks(N2)) + lr::BS_SLOTS) * sizeof(double)))
        return fail(LR_ERR_NOMEM, "lr_bridge_solve: allocating the workspaces of %lld + %lld terms failed", (long long)N1, (long long)N2);
    if (!on_device) {
        LR_HIP(hipMemcpyAsync(d1.p, l1, (size_t)N1 * sizeof(double), hipMemcpyHostToDevice, st));
        LR_HIP(hipMemcpyAsync(d2.p, l2, (size_t)N2 * sizeof(double), hipMemcpyHostToDevice, st));
        l1 = static_cast<const double*>(d1.p);
        l2 = static_cast<const double*>(d2.p);
    }
    const int rc = bridge_solve(l1, N1, l2, N2, n_eff, tol, maxit, static_cast<double*>(dit.p), st, table);
    (void)hipStreamSynchronize(st);  // the workspaces are freed on return
    return rc;
}

// ---- device memory / stream / event helpers -------------------------------------------------------
int lr_malloc(int device, uint64_t bytes, void** dptr) {
    if (!dptr) return fail(LR_ERR_INVALID, "dptr is NULL");
    LR_HIP(hipSetDevice(device));
    if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess) return fail(LR_ERR_NOMEM, "hipMalloc(%llu) failed", (unsigned long long)bytes);
    return LR_OK;
}
int lr_free(int device, void* dptr) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipFree(dptr));
    return LR_OK;
}
int lr_memcpy_h2d(int device, void* dst, const void* src, uint64_t bytes, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    LR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return LR_OK;
}
int lr_memcpy_d2h(int device, void* dst, const void* src, uint64_t bytes, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    LR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return LR_OK;
}
int lr_memset(int device, void* dst, int value, uint64_t bytes, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
    return LR_OK;
}
int lr_stream_create(int device, void** stream) {
    if (!stream) return fail(LR_ERR_INVALID, "stream is NULL");
    LR_HIP(hipSetDevice(device));
    hipStream_t s;
    LR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return LR_OK;
}
int lr_stream_destroy(int device, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipStreamDestroy((hipStream_t)stream));
    return LR_OK;
}
int lr_stream_sync(int device, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return LR_OK;
}
int lr_event_create(int device, void** event) {
    if (!event) return fail(LR_ERR_INVALID, "event is NULL");
    LR_HIP(hipSetDevice(device));
    hipEvent_t e;
    LR_HIP(hipEventCreate(&e));
    *event = e;
    return LR_OK;
}
int lr_event_destroy(int device, void* event) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipEventDestroy((hipEvent_t)event));
    return LR_OK;
}
int lr_event_record(int device, void* event, void* stream) {
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return LR_OK;
}
int lr_event_elapsed_ms(int device, void* start, void* stop, float* ms) {
    if (!ms) return fail(LR_ERR_INVALID, "ms is NULL");
    LR_HIP(hipSetDevice(device));
    LR_HIP(hipEventSynchronize((hipEvent_t)stop));
    LR_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return LR_OK;
}

// ---- the C-level exchange: RCCL, resolved at first use (no link-time dependency; see include/logreg_hip.h)
}  // extern "C"
#include <dlfcn.h>
// (RCCL's header only where the ROCm installation has it -- the library is resolved with dlopen at first use either way; without the
//  header, the handful of declarations this file needs, with the ABI values of rccl.h)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint8 = 1, ncclDouble = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
ncclResult_t ncclGetUniqueId(ncclUniqueId*);
ncclResult_t ncclCommInitRank(ncclComm_t*, int, ncclUniqueId, int);
ncclResult_t ncclCommDestroy(ncclComm_t);
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();
ncclResult_t ncclSend(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ncclRecv(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ncclAllReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
const char* ncclGetErrorString(ncclResult_t);
}
#endif
struct lr_comm {
    ncclComm_t comm;
    int rank, world, device;
};
namespace {
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.h) return LR_OK;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) return fail(LR_ERR_UNSUPPORTED, "RCCL (librccl.so.1) could not be loaded: %s", dlerror());
    Rccl r;
    r.h = h;
#define LR_SYM(field, name)                                                     \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(h, name));              \
    if (!r.field) return fail(LR_ERR_UNSUPPORTED, "RCCL symbol %s not found", name);
    LR_SYM(get_unique_id, "ncclGetUniqueId")
    LR_SYM(comm_init_rank, "ncclCommInitRank")
    LR_SYM(comm_destroy, "ncclCommDestroy")
    LR_SYM(group_start, "ncclGroupStart")
    LR_SYM(group_end, "ncclGroupEnd")
    LR_SYM(send, "ncclSend")
    LR_SYM(recv, "ncclRecv")
    LR_SYM(all_reduce, "ncclAllReduce")
    LR_SYM(error_string, "ncclGetErrorString")
#undef LR_SYM
    g_rccl = r;
    return LR_OK;
}
#define LR_NCCL(call)                                                                                       \
    do {                                                                                                    \
        const ncclResult_t r_ = (call);                                                                     \
        if (r_ != ncclSuccess) return fail(LR_ERR_HIP, "%s failed: %s", #call, g_rccl.error_string(r_));    \
    } while (0)
}  // namespace
extern "C" {

int lr_comm_unique_id(void* id) {
    static_assert(LR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "identifier size");
    if (!id) return fail(LR_ERR_INVALID, "id is NULL");
    if (int rc = rccl_load()) return rc;
    ncclUniqueId u;
    LR_NCCL(g_rccl.get_unique_id(&u));
    std::memcpy(id, u.internal, LR_COMM_ID_BYTES);
    return LR_OK;
}
int lr_comm_create(const void* id, int32_t rank, int32_t world, int device, lr_comm** out) {
    if (!id || !out) return fail(LR_ERR_INVALID, "id / out is NULL");
    if (world < 1 || rank < 0 || rank >= world) return fail(LR_ERR_INVALID, "rank %d of world %d", rank, world);
    if (int rc = rccl_load()) return rc;
    LR_HIP(hipSetDevice(device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, LR_COMM_ID_BYTES);
    ncclComm_t c;
    LR_NCCL(g_rccl.comm_init_rank(&c, world, u, rank));
    *out = new lr_comm{c, rank, world, device};
    return LR_OK;
}
int lr_comm_destroy(lr_comm* comm) {
    if (!comm) return LR_OK;
    if (g_rccl.h) (void)g_rccl.comm_destroy(comm->comm);
    delete comm;
    return LR_OK;
}
int lr_gather(lr_comm* comm, const void* send, void* recv, uint64_t bytes, int32_t root, void* stream) {
    if (!comm || !send) return fail(LR_ERR_INVALID, "comm / send is NULL");
    if (root < 0 || root >= comm->world) return fail(LR_ERR_INVALID, "root %d of world %d", root, comm->world);
    if (comm->rank == root && !recv) return fail(LR_ERR_INVALID, "recv is NULL on the root rank");
    LR_HIP(hipSetDevice(comm->device));
    // every rank sends its block to the root, the root receives world blocks in rank order: ONE group (xGMI point-to-point)
    LR_NCCL(g_rccl.group_start());
    LR_NCCL(g_rccl.send(send, bytes, ncclUint8, root, comm->comm, (hipStream_t)stream));
    if (comm->rank == root)
        for (int r = 0; r < comm->world; ++r)
            LR_NCCL(g_rccl.recv(static_cast<unsigned char*>(recv) + (uint64_t)r * bytes, bytes, ncclUint8, r, comm->comm, (hipStream_t)stream));
    LR_NCCL(g_rccl.group_end());
    return LR_OK;
}
int lr_allreduce_sum_f64(lr_comm* comm, double* buf, uint64_t count, void* stream) {
    if (!comm || !buf) return fail(LR_ERR_INVALID, "comm / buf is NULL");
    LR_HIP(hipSetDevice(comm->device));
    LR_NCCL(g_rccl.all_reduce(buf, buf, count, ncclDouble, ncclSum, comm->comm, (hipStream_t)stream));
    return LR_OK;
}

}  // extern "C"
