// lr_engine.h -- the host side between the C ABI (lr_api.hip) and the kernel launches: packs the by-value kernel argument structs
// from a model handle, a plan (lr_plan.h) and the caller's options, owns the stepwise engine's workspace and states its launches
// (load -> partial -> update per evaluation; the interior leapfrog steps as the StepwisePlan of lr_plan.h says: which kernel runs, on
// which slicing, is decided there).  No arithmetic of the path and no choice of a kernel happens here.  Included once, by lr_api.hip
// (after lr_model.h and lr_plan.h).
#pragma once

namespace {

template <typename T, int P> lr::ModelArgs<T, P> model_args(const lr_model* m) {
    lr::ModelArgs<T, P> a{};
    a.rows = static_cast<const T*>(m->d_rows);
    a.rows_tw = static_cast<const float*>(m->d_rows_tw);
    a.rows_mf = static_cast<const float*>(m->d_xmf);
    a.ops_mf = static_cast<const unsigned char*>(m->d_xms);
    a.n = m->n;
    for (int j = 0; j < P; ++j) a.prior.inv_var[j] = (T)m->inv_var[j];
    a.prior.lprior_const = m->lprior_const;
    return a;
}

struct RunSpec {
    int kind;
    double step;
    int l;
    double a[kMaxP], b[kMaxP], c[kMaxP];
};

// step and per-coordinate vectors of a run in the kernels' type (ChainArgs, TallArgs)
template <typename T, int P, typename Args> void fill_tuning(const RunSpec& rs, Args* a) {
    a->step = (T)rs.step;
    for (int j = 0; j < P; ++j) a->a[j] = (T)rs.a[j], a->b[j] = (T)rs.b[j], a->c[j] = (T)rs.c[j];
}

template <typename T, int P>
int do_eval_t(lr_model* m, const Plan& pl, hipStream_t st, int64_t C, const void* beta, void* ll, void* lprior,
              void* lpost, void* grad) {
    auto ma = model_args<T, P>(m);
    lr::EvalArgs<T> ea;
    ea.beta = static_cast<const T*>(beta);
    ea.C = C;
    ea.p = m->p;
    ea.ll = static_cast<T*>(ll);
    ea.lprior = static_cast<T*>(lprior);
    ea.lpost = static_cast<T*>(lpost);
    ea.grad = static_cast<T*>(grad);
    lr::LaunchCfg cfg{pl.mode, pl.G, pl.R, 0, st, pl.lds_bytes, m->dbg.residency_cap ? m->cus : 0};
    const int rc = m->table->launch_eval(&cfg, C, &ma, &ea);
    if (rc != 0) return fail(rc == -3 ? LR_ERR_UNSUPPORTED : LR_ERR_HIP, "eval launch failed (%d): %s", rc,
                             hipGetErrorString(hipGetLastError()));
    return LR_OK;
}

template <typename T, int P>
int do_chain_t(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, void* state,
               double* lp_state, void* out, uint32_t* accepts) {
    auto ma = model_args<T, P>(m);
    lr::ChainArgs<T, P> ca{};
    ca.state = static_cast<T*>(state);
    ca.lp_state = lp_state;
    ca.out = static_cast<T*>(out);
    ca.accepts = accepts;
    ca.C = o->n_chains;
    ca.chain_offset = o->chain_offset;
    ca.iters = o->iters;
    ca.thin = o->thin;
    ca.iter_offset = o->iter_offset;
    ca.seed = o->seed;
    ca.p = m->p;
    ca.l = rs.l;
    fill_tuning<T, P>(rs, &ca);
    for (int j = 0; j < P; ++j) {
        const double ks = sizeof(T) == 4 ? 1.4426950408889634 : 1.0;  // lr::ExpScale<T>::k
        ca.d[j] = (T)(rs.b[j] * ks);
        ca.e[j] = (T)(m->inv_var[j] / ks);
    }
    ca.stats = lr::StatsArgs{o->stats, o->stats_batch, o->stats_first};
    ca.interior_bf16 = rs.kind == lr::KIND_HMC && pl.mode == lr::MODE_MFMA && o->precision != LR_PREC_FULL;
    // a plan in two parts: chains whose position in the PLANNED run is below pl.split go to (G, R), the rest to (G2, R2)
    const int64_t C = o->n_chains, pos0 = o->plan_chains > 0 ? o->chain_offset - o->plan_first : 0;
    const int64_t head = pl.split > 0 ? (pl.split - pos0 < 0 ? 0 : (pl.split - pos0 > C ? C : pl.split - pos0)) : C;
    // Both parts present: the remainder runs CO-RESIDENT with the head, on the handle's side stream -- fork from the caller's
    // stream (everything enqueued so far), join back into it.  The head is VALU-issue-bound on one wave per SIMD, the remainder
    // (wide lane groups) mostly waits on cross-lane reductions: together 0.542 instead of 0.639 ms per step at 5120 chains
    // (profiles/r4_two_part_corun.txt, r4_two_part_check.txt).  The head keeps its residency cap (one workgroup per CU); the
    // remainder asks for none, so that it fits beside the head.
    // ... while the head is at most two waves per SIMD: beside a head of three the remainder only gets in the way (HMC, 13 312 chains:
    // 1.32 ms back to back, 1.47 co-resident, 1.40 as one launch; profiles/r4_chain_grid_corun_all.txt) -- then the parts run in turn
    const bool two = head > 0 && head < C;
    // (the threaded-ll kernels gain from the overlap at three waves as well: MALA +6 %, RWMH +10 % co-resident against -2 % / -1 % in turn)
    // (a matrix-core head: workgroups per CU instead -- 16 chains per workgroup at S >= 4, 64 at S = 1)
    const int64_t head_rounds = pl.mode == lr::MODE_MFMA ? head / ((pl.G == 1 ? 64 : 16) * (int64_t)m->cus) : head * pl.G / 64 / (4LL * m->cus);
    const bool both = two && pl.corun && (rs.kind != lr::KIND_HMC || head_rounds <= 2);
    lr_model::Side* side_slot = nullptr;
    if (both) {
        for (auto& e : m->sides)
            if (e.caller == st) side_slot = &e;
        if (!side_slot) {  // created all or nothing: a partly made slot is destroyed again, never kept
            lr_model::Side e{st, nullptr, nullptr, nullptr};
            const bool ok = hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking) == hipSuccess &&
                            hipEventCreateWithFlags(&e.ev_fork, hipEventDisableTiming) == hipSuccess &&
                            hipEventCreateWithFlags(&e.ev_join, hipEventDisableTiming) == hipSuccess;
            if (!ok) {
                const hipError_t err = hipGetLastError();
                if (e.ev_join) (void)hipEventDestroy(e.ev_join);
                if (e.ev_fork) (void)hipEventDestroy(e.ev_fork);
                if (e.stream) (void)hipStreamDestroy(e.stream);
                return fail(LR_ERR_HIP, "creating the side stream of a two-part launch failed: %s", hipGetErrorString(err));
            }
            m->sides.push_back(e);
            side_slot = &m->sides.back();
        }
        if (hipEventRecord(side_slot->ev_fork, st) != hipSuccess || hipStreamWaitEvent(side_slot->stream, side_slot->ev_fork, 0) != hipSuccess)
            return fail(LR_ERR_HIP, "forking the two-part launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    for (int part = 0; part < 2; ++part) {
        ca.first = part == 0 ? 0 : head;
        ca.count = part == 0 ? head : C - head;
        if (ca.count <= 0) continue;
        const bool side = both && part == 1;
        lr::LaunchCfg cfg{part == 0 ? pl.mode : pl.mode2, part == 0 ? pl.G : pl.G2, part == 0 ? pl.R : pl.R2, rs.kind, side ? side_slot->stream : st,
                          part == 0 || pl.mode2 == lr::MODE_MIXED ? pl.lds_bytes : 0, m->dbg.residency_cap && !side ? m->cus : 0};
        const int rc = m->table->launch_chain(&cfg, ca.count, &ma, &ca);
        if (rc != 0) return fail(rc == -3 ? LR_ERR_UNSUPPORTED : LR_ERR_HIP, "chain launch failed (%d): %s", rc,
                                 hipGetErrorString(hipGetLastError()));
    }
    if (both) {
        if (hipEventRecord(side_slot->ev_join, side_slot->stream) != hipSuccess || hipStreamWaitEvent(st, side_slot->ev_join, 0) != hipSuccess)
            return fail(LR_ERR_HIP, "joining the two-part launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    return LR_OK;
}

// ---- the stepwise engine.  A run's argument block is filled ONCE -- setup_tall: model, StepwisePlan (lr_plan.h), workspace; then the
// caller's arrays -- and is const from then on.  Every launch goes through TallRun::issue, which copies the block, applies what THAT
// launch differs in (TallOver) and calls the table: no field is ever set for a launch and put back after it.
template <typename T, int P>
int setup_tall(lr_model* m, const StepwisePlan& sp, hipStream_t st, int64_t C, lr::TallArgs<T, P>* pa, size_t extra = 0, unsigned char** extra_out = nullptr) {
    // C: chains of this call (sizes the workspace and the grids; the plan was made for the run's: plan_count)
    // extra: bytes the caller carves itself, behind the engine's own pieces of the same block (NUTS: lr_nuts_sched.h)
    // (chain blocks of 16 .. 128 chains are the grid's y / x dimension of the partial kernels: y is a 16-bit quantity)
    if ((C + 63) / 64 > 65535) return fail(LR_ERR_UNSUPPORTED, "the stepwise engine takes at most %lld chains per call (got %lld): split the run into shards (chain_offset)", 65535LL * 64, (long long)C);
    // every field starts from zero: the flags only some launches set (part_f32, fuse_mid, interior) were once left to whatever the
    // caller's stack held -- found in round 5 when a float64 run on the trajectory kernels, which never touches part_f32, now and then
    // had its end-point update read float64 partials as float32
    lr::TallArgs<T, P>& a = *pa = lr::TallArgs<T, P>{};
    auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t vec = align((size_t)C * P * sizeof(T)), dbl = align((size_t)C * sizeof(double));
    const int RSmax = sp.RS_i > sp.RS ? sp.RS_i : sp.RS;
    const size_t pg = align((size_t)RSmax * C * P * sizeof(T)), cv = align((size_t)2 * P * sizeof(T));
    // (second state pair + second partial buffer: the fused interior steps of the row-split kernels; constants)
    const size_t need = 4 * vec + 2 * dbl + align((size_t)C * 4) + pg + align((size_t)sp.RS * C * sizeof(double)) + (sp.alt_buffers ? 2 * vec + pg : 0) + cv + extra;
    lr_model::Ws* slot = nullptr;
    for (auto& e : m->ws)
        if (e.stream == st) slot = &e;
    if (!slot) {
        if (m->ws.size() >= 16) {  // a caller cycling through streams: drop every workspace once all work is done
            if (hipDeviceSynchronize() != hipSuccess) return fail(LR_ERR_HIP, "hipDeviceSynchronize failed");
            for (auto& e : m->ws)
                if (e.p) (void)hipFree(e.p);
            m->ws.clear();
        }
        m->ws.push_back({st, nullptr, 0});
        slot = &m->ws.back();
    }
    if (need > slot->bytes) {
        if (slot->p) (void)hipFree(slot->p);  // (work already enqueued on this stream may still use the old block: hipFree waits for the device)
        slot->p = nullptr, slot->bytes = 0;
        if (hipMalloc(&slot->p, need) != hipSuccess) return fail(LR_ERR_NOMEM, "stepwise workspace of %zu bytes", need);
        slot->bytes = need;
    }
    unsigned char* w = static_cast<unsigned char*>(slot->p);
    auto carve = [&](size_t b) { unsigned char* r = w; w += b; return r; };
    a.rows = static_cast<const T*>(m->d_rows);
    a.rows_tw = static_cast<const float*>(m->d_rows_tw);
    a.n = m->n, a.C = C, a.p = m->p;
    a.slice_len = sp.slice_len, a.RS = sp.RS;
    for (int j = 0; j < P; ++j) a.prior.inv_var[j] = (T)m->inv_var[j];
    a.prior.lprior_const = m->lprior_const;
    a.x = (T*)carve(vec), a.g = (T*)carve(vec);
    a.q1 = (T*)carve(vec), a.pm = (T*)carve(vec);
    a.lp = (double*)carve(dbl), a.aux = (double*)carve(dbl);
    a.nacc = (uint32_t*)carve(align((size_t)C * 4));
    a.part_g = (T*)carve(pg);
    a.RS_i = sp.bf16_interior ? sp.RS_i : 0;
    a.traj_tiles = sp.traj_tiles, a.traj_fmt = sp.traj_fmt;
    a.slice_len_i = sp.slice_len_i, a.rowsplit_waves = sp.waves;
    a.part_v = (double*)carve(align((size_t)sp.RS * C * sizeof(double)));
    a.cvec = (const T*)carve(cv);
    if (sp.alt_buffers) {  // the second pair: a launch's *_in buffers (TallOver::cur says which pair is which)
        a.q1_in = (const T*)carve(vec);
        a.pm_in = (const T*)carve(vec);
        a.part_in = (const T*)carve(pg);
    }
    if (extra_out) *extra_out = carve(extra);
    a.wide_bf16 = sp.wide_engine;
    a.xblk = static_cast<const uint16_t*>(m->d_xblk), a.xmx = static_cast<const uint16_t*>(m->d_xmx);
    a.xblk1 = static_cast<const uint16_t*>(m->d_xblk1), a.xblk1h = static_cast<const uint16_t*>(m->d_xblk1h);
    return LR_OK;
}
// ... and what every sampler adds to it
template <typename T, int P>
void sampler_args(const RunSpec& rs, const lr_run_opts* o, void* state, void* out, lr::TallArgs<T, P>* a) {
    a->state = static_cast<T*>(state);
    a->out = static_cast<T*>(out);
    a->chain_offset = o->chain_offset;
    a->seed = o->seed;
    a->l = rs.l;
    fill_tuning<T, P>(rs, a);
    a->stats = lr::StatsArgs{o->stats, o->stats_batch, o->stats_first};
}

// what one launch differs in from the run's argument block; the defaults are an exact kernel on the first buffer pair
struct TallOver {
    int cur = 0;           // which of the two (q1, pm, part_g) sets is current: the other one is this launch's (q1_in, pm_in, part_in)
    int RS = 0;            // slice partials an update sums, where the interior kernel just wrote another count than the exact one (0: the exact)
    int interior = 0;      // an interior HMC gradient evaluation that runs in reduced precision
    int part_f32 = 0;      // float64 models: the partials this update reads are float32 (an interior kernel wrote them)
    int fuse_mid = 0;      // the interior kernel first finishes the previous leapfrog step from the *_in buffers
    bool stamped = false;  // development builds: the launch records time stamps (lr_stamps.h)
};
template <typename T, int P> struct TallRun {
    const lr::InstTable* t;
    hipStream_t st;
    const lr::TallArgs<T, P> base;
    int rc = 0;  // of the first launch that failed: nothing is launched after it
    template <typename F> void issue(const TallOver& o, F&& launch) {
        if (rc) return;
        lr::TallArgs<T, P> a = base;
        if (o.cur) {
            a.q1 = const_cast<T*>(base.q1_in), a.pm = const_cast<T*>(base.pm_in), a.part_g = const_cast<T*>(base.part_in);
            a.q1_in = base.q1, a.pm_in = base.pm, a.part_in = base.part_g;
        }
        if (o.RS) a.RS = o.RS;
        a.interior = o.interior, a.part_f32 = o.part_f32, a.fuse_mid = o.fuse_mid;
        if (o.stamped) LR_STAMPS_ARM(a);
        rc = launch(&a);
    }
    void partial(int value, int grad, const TallOver& o = {}) { issue(o, [&](const void* a) { return t->launch_tall_partial(st, value, grad, a); }); }
    void update(int kind, int phase, int64_t iter, int64_t out_row, int next, const TallOver& o = {}) { issue(o, [&](const void* a) { return t->launch_tall_update(st, kind, phase, iter, out_row, next, a); }); }
};

// lr_eval through the stepwise engine (tall or wide models): load -> partial(value, grad) -> finish
template <typename T, int P>
int do_eval_stepwise_t(lr_model* m, const Plan& pl, hipStream_t st, int64_t C, const void* beta, void* ll, void* lprior,
                       void* lpost, void* grad) {
    lr::TallArgs<T, P> a;
    const int rc = setup_tall<T, P>(m, plan_stepwise(m, pl, -1, 0, LR_PREC_FULL, C), st, C, &a);
    if (rc) return rc;
    a.state = static_cast<T*>(const_cast<void*>(beta));
    a.ev_ll = static_cast<T*>(ll);
    a.ev_lprior = static_cast<T*>(lprior);
    a.ev_lpost = static_cast<T*>(lpost);
    a.ev_grad = static_cast<T*>(grad);
    TallRun<T, P> run{m->table, st, a};
    run.update(lr::KIND_HMC, lr::PH_LOAD, 0, -1, 0);
    run.partial(1, 1);
    run.update(lr::KIND_HMC, lr::PH_EVAL, 0, -1, 0);
    if (run.rc) return fail(LR_ERR_HIP, "stepwise eval launch failed (%d): %s", run.rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}

template <typename T, int P>
int do_stepwise_t(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, void* state,
                  double* lp_state, void* out, uint32_t* accepts) {
    const int kind = rs.kind;
    const StepwisePlan sp = plan_stepwise(m, pl, kind, rs.l, o->precision, plan_count(o));
    lr::TallArgs<T, P> a;
    const int rc = setup_tall<T, P>(m, sp, st, o->n_chains, &a);
    if (rc) return rc;
    sampler_args<T, P>(rs, o, state, out, &a);
    a.lp_state = lp_state;
    a.accepts = accepts;
    TallRun<T, P> run{m->table, st, a};
    // The launches of this run, each with all it differs in.  `cur` moves only on PATH_FUSED; where it stands when a trajectory ends
    // is where the next one, PH_END and PH_STORE find the state.
    int cur = 0;
    auto exact = [&] { TallOver v; v.cur = cur; return v; };
    auto interior = [&](int fused) {  // an interior leapfrog gradient: reduced precision where the plan says so
        TallOver v = exact();
        v.interior = sp.bf16_interior, v.fuse_mid = fused, v.stamped = true;
        return v;
    };
    auto mid = [&] {  // the update behind interior steps: as many slice partials as the interior kernel wrote, float32 ones on a float64 model
        TallOver v = exact();
        v.RS = sp.RS_mid(), v.part_f32 = sizeof(T) == 8 && sp.bf16_interior;
        return v;
    };
    run.update(kind, lr::PH_LOAD, 0, -1, 0);
    if (kind == lr::KIND_HMC) run.partial(1, 1);
    else if (kind != lr::KIND_RWMH) run.partial(0, 1);
    run.update(kind, lr::PH_INIT, o->iter_offset, -1, 0);
    const int64_t total = o->iters * o->thin;
    const int steps = kind == lr::KIND_HMC ? rs.l - 1 : 0;  // interior leapfrog steps of an iteration
    for (int64_t tt = 0; tt < total && !run.rc; ++tt) {
        if (sp.path == PATH_TRAJ) {  // (planned for HMC with L > 1 only)
            TallOver v = exact();
            v.stamped = true;
            run.issue(v, [&](const void* p) { return m->table->launch_tall_traj(st, p); });
        } else if (sp.path == PATH_FUSED) {
            for (int i = 0; i < steps; ++i) {
                if (i > 0) cur ^= 1;  // the launch reads the step it finishes from the pair the previous launch wrote
                run.partial(0, 1, interior(i > 0));
            }
            if (steps > 0) run.update(kind, lr::PH_MID, 0, -1, 0, mid());
        } else {  // PATH_PER_STEP, PATH_EXACT
            for (int i = 0; i < steps; ++i) {
                run.partial(0, 1, interior(0));
                run.update(kind, lr::PH_MID, 0, -1, 0, mid());
            }
        }
        if (kind == lr::KIND_HMC || kind == lr::KIND_MALA) run.partial(1, 1, exact());
        else if (kind == lr::KIND_RWMH) run.partial(1, 0, exact());
        else run.partial(0, 1, exact());
        const int64_t out_row = ((tt + 1) % o->thin == 0) ? (tt + 1) / o->thin - 1 : -1;
        run.update(kind, lr::PH_END, o->iter_offset + tt, out_row, tt + 1 < total, exact());
    }
    run.update(kind, lr::PH_STORE, 0, -1, 0, exact());
    if (run.rc) return fail(LR_ERR_HIP, "stepwise launch failed (%d): %s", run.rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}

// NUTS on the stepwise engine (lr_tall_nuts.h; the schedule: lr_nuts_sched.h).  Per iteration: for every leaf the evaluation at q1 and
// the leaf's update launch.  The one thing the host learns from the device is how many chains are still building, read at the end of
// a doubling on the caller's stream (at most max_depth - 1 waits per iteration); zero ends the iteration.  The loop is bounded by
// 2^max_depth - 1 leaves whatever it reads, and a finished chain is inert, so the results do not depend on when the host looks.
// Full precision at every leaf: the plan of a NUTS run is PATH_EXACT.
//
// A warm-up (NutsWarm; include/logreg_hip_adapt_tall.h) is the same loop on the TUNED kernel: the tuning comes from `tune`, every
// iteration ends with flag = 0 and writes its acceptance statistics, `after` enqueues what rewrites the tuning block, and the next
// iteration begins from the carried state as a launch of its own (NPH_CARRY), which reads the new tuning.
struct NutsWarm {
    const void* tune;  // NutsTune<T, P> in device memory
    std::function<double*(int64_t)> astat;  // [C] of the call's iteration i
    std::function<int(int64_t, const void* x, int64_t ld, const double* astat)> after;  // behind iteration i's end; x: the states [C][ld]
};
template <typename T, int P>
int do_nuts_stepwise_t(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, int max_depth, void* state, void* out,
                       void* counters, int8_t* depth_out, const NutsWarm* warm) {
    const int64_t C = o->n_chains;
    const lr::InstTable* t = m->table;
    if (!t->launch_tall_nuts || !t->launch_tall_nuts_tuned) return fail(LR_ERR_UNSUPPORTED, "NUTS: no stepwise kernel for padded p = %d", m->P);
    const lr::NutsTallCarve cv = lr::nuts_tall_carve(C, P, sizeof(T), max_depth);
    lr::TallArgs<T, P> a;
    unsigned char* w = nullptr;
    const int rc = setup_tall<T, P>(m, plan_stepwise(m, pl, LR_KIND_NUTS, 0, o->precision, plan_count(o)), st, C, &a, cv.total, &w);
    if (rc) return rc;
    sampler_args<T, P>(rs, o, state, out, &a);
    TallRun<T, P> run{t, st, a};
    const lr::NutsTallArgs<T> na{reinterpret_cast<T*>(w + cv.vec_off), reinterpret_cast<lr::NutsTallChain*>(w + cv.chain_off), reinterpret_cast<uint32_t*>(w + cv.tally_off),
                                 static_cast<lr::NutsCounters*>(counters), depth_out, max_depth};
    lr::NutsTallTunedArgs<T, P> nt{na, warm ? static_cast<const lr::NutsTune<T, P>*>(warm->tune) : nullptr, nullptr};
    auto N = [&](int phase, int64_t iter, const lr::NutsStep& leaf, int64_t out_row, int flag) {
        run.issue({}, [&](const void* p) {
            return warm ? t->launch_tall_nuts_tuned(st, p, &nt, phase, iter, leaf.s, leaf.d, leaf.i, out_row, flag)
                        : t->launch_tall_nuts(st, p, &na, phase, iter, leaf.s, leaf.d, leaf.i, out_row, flag);
        });
    };
    const lr::NutsStep none{};
    run.update(lr::KIND_HMC, lr::PH_LOAD, 0, -1, 0);
    run.partial(1, 1);
    N(lr::NPH_BEGIN, o->iter_offset, none, -1, 1);
    const int64_t total = o->iters * o->thin;
    for (int64_t tt = 0; tt < total && !run.rc; ++tt) {
        if (warm) {
            nt.astat = warm->astat(tt);
            if (tt > 0) N(lr::NPH_CARRY, o->iter_offset + tt, none, -1, 0);
        }
        for (lr::NutsSched sch(max_depth); !sch.done() && !run.rc;) {
            const lr::NutsStep leaf = sch.cur();
            run.partial(1, 1);
            N(lr::NPH_LEAF, o->iter_offset + tt, leaf, -1, leaf.read);
            uint32_t building = 1;
            if (leaf.read && !run.rc) {
                if (hipMemcpyAsync(&building, na.tally + leaf.d, sizeof(building), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                    return fail(LR_ERR_HIP, "NUTS: reading the tally of building chains failed: %s", hipGetErrorString(hipGetLastError()));
            }
            sch.advance(building);
        }
        const int64_t out_row = ((tt + 1) % o->thin == 0) ? (tt + 1) / o->thin - 1 : -1;
        N(lr::NPH_END, o->iter_offset + tt, none, out_row, !warm && tt + 1 < total);
        if (warm && !run.rc)
            if (const int rca = warm->after(tt, a.x, P, nt.astat)) return rca;
    }
    N(lr::NPH_STORE, 0, none, -1, 0);
    if (run.rc) return fail(LR_ERR_HIP, "stepwise NUTS launch failed (%d): %s", run.rc, hipGetErrorString(hipGetLastError()));
    return LR_OK;
}

int bad_width(const lr_model* m) { return fail(LR_ERR_UNSUPPORTED, "unsupported padded width %d", m->P); }

int do_eval_stepwise(lr_model* m, const Plan& pl, hipStream_t st, int64_t C, const void* beta, void* ll, void* lprior,
                     void* lpost, void* grad);

int do_eval(lr_model* m, const Plan& pl, hipStream_t st, int64_t C, const void* beta, void* ll, void* lprior,
            void* lpost, void* grad) {
    if (pl.mode == lr::MODE_STEPWISE) return do_eval_stepwise(m, pl, st, C, beta, ll, lprior, lpost, grad);
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, do_eval_t, m, pl, st, C, beta, ll, lprior, lpost, grad)
    return bad_width(m);
}

int do_stepwise(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, void* state,
                double* lp_state, void* out, uint32_t* accepts) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, m->dtype, m->P, do_stepwise_t, m, pl, st, rs, o, state, lp_state, out, accepts)
    return bad_width(m);
}

int do_eval_stepwise(lr_model* m, const Plan& pl, hipStream_t st, int64_t C, const void* beta, void* ll, void* lprior,
                     void* lpost, void* grad) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, m->dtype, m->P, do_eval_stepwise_t, m, pl, st, C, beta, ll, lprior, lpost, grad)
    return bad_width(m);
}

int do_nuts_stepwise(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, int max_depth, void* state, void* out, void* counters,
                     int8_t* depth_out, const NutsWarm* warm = nullptr) {
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_ALL, m->dtype, m->P, do_nuts_stepwise_t, m, pl, st, rs, o, max_depth, state, out, counters, depth_out, warm)
    return bad_width(m);
}

int do_chain(lr_model* m, const Plan& pl, hipStream_t st, const RunSpec& rs, const lr_run_opts* o, void* state,
             double* lp_state, void* out, uint32_t* accepts) {
    if (pl.mode == lr::MODE_STEPWISE) return do_stepwise(m, pl, st, rs, o, state, lp_state, out, accepts);
    LR_RETURN_BY_DTYPE_WIDTH(LR_WIDTHS_FUSED, m->dtype, m->P, do_chain_t, m, pl, st, rs, o, state, lp_state, out, accepts)
    return bad_width(m);
}

}  // namespace
