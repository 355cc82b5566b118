// Shared machinery of the trajectory drivers (traj.hip, traj_systems.hip).
#pragma once

#include <chrono>

#include "femfct_internal.h"
#include "device_utils.h"
#include "forms.h"

#include <algorithm>
#include <stdio.h>
#include <stdlib.h>

int femfct_ensure_traj_ws(femfct_ctx* ctx, int32_t batch, int32_t steps);
int femfct_ensure_krylov_ws(femfct_ctx* ctx, int32_t batch);
int femfct_enqueue_step_end(femfct_ctx* ctx, int delta, int32_t batch, bool with_krylov);
void femfct_request_fused_end(femfct_ctx* ctx, int delta, bool with_krylov);
int femfct_enqueue_step_ref(femfct_ctx* ctx, const double* A, const double* N, int32_t nshared, VecRef rhs,
                            int64_t rhs_bstride, VecRef u_n, int64_t u_bstride, double dt, VecRef u_out,
                            int64_t out_bstride, int32_t batch, int32_t budget);
int femfct_enqueue_step_mat(femfct_ctx* ctx, MatRef A, const double* N, int32_t nshared, VecRef rhs, int64_t rhs_bstride,
                            VecRef u_n, int64_t u_bstride, double dt, VecRef u_out, int64_t out_bstride, int32_t batch,
                            int32_t budget);
int femfct_enqueue_axpby(femfct_ctx* ctx, int64_t count, double alpha, const double* a, double beta, const double* b,
                         double* out);
struct SbOpArgs;
bool femfct_inline_ops_wanted(const femfct_ctx* ctx, int32_t batch);
int femfct_enqueue_step_op(femfct_ctx* ctx, MatRef A, const SbOpArgs* sb, const double* N, int32_t nshared, VecRef rhs,
                           int64_t rhs_bstride, VecRef u_n, int64_t u_bstride, double dt, VecRef u_out, int64_t out_bstride,
                           int32_t batch, int32_t budget);

static inline int femfct_round_kry_budget(const femfct_ctx* ctx, int b) {
    b = (b + 3) & ~3;
    if (b < 4) b = 4;
    if (b > ctx->kry_max_iters) b = ctx->kry_max_iters;
    return b;
}

// Captured graph holding `reps` consecutive, identical time steps (the time level is a device counter).
template <class F>
int femfct_run_graph_reps(femfct_ctx* ctx, femfct_ctx::GraphKey key, int reps, int delta, F&& enqueue_one) {
    key.push_back(key_bits((int32_t)reps));
    key.push_back(key_bits((int32_t)ctx->pair_rows));     // a different Jacobi kernel is captured
    key.push_back(key_bits((int32_t)ctx->solver));
    key.push_back(key_bits(ctx->low_src));                 // the tile step reads pre-built L_k / D_k (femfct_prebuild_low)
    key.push_back(key_bits(ctx->low_dt));
    key.push_back(key_bits((int32_t)(ctx->tile_lean | ctx->tile_cone << 1 | ctx->tile_fit << 2 | femfct_tile_trim_mask(ctx) << 3)));   // other sweep loops / patches of the tile kernels are captured
    // delta: the time-level step of this kind of sweep (+1 forward, -1 adjoint).  Step r is enqueued with its level
    // offset baked into every level-indirected reference (lref, MatRef::level_off); the device counters move once, in
    // the last step of the graph -- no per-step ticket / counter update on the critical path of the other R - 1 steps.
    struct Restore {
        femfct_ctx* c;
        ~Restore() { c->level_bias = 0; c->ord_bias = 0; c->rep_total = 1; c->rep_last = true; }
    } restore{ctx};
    return femfct_run_graph(ctx, key, [&]() {
        for (int r = 0; r < reps; ++r) {
            ctx->level_bias = r * delta; ctx->ord_bias = r; ctx->rep_total = reps; ctx->rep_last = (r == reps - 1);
            int rc = enqueue_one();
            if (rc != FEMFCT_OK) return rc;
        }
        return (int)FEMFCT_OK;
    });
}

// level-indirected reference of the step being enqueued (see femfct_run_graph_reps)
static inline VecRef lref(const femfct_ctx* ctx, const double* p, const int32_t* level, int64_t stride, int32_t off) {
    return make_ref(p, level, stride, off + (level ? ctx->level_bias : 0));
}

// ---- the sweep controller (sweep_ctl.hip): plan -> run -> verdict, repeated until the sweep is accepted or fails ----
struct SweepSpec {
    SweepKind kind;
    int32_t num_steps, batch;
    int level0;         // time level the device counter starts from
    bool krylov;        // the step has a species solve (its log is read too)
    bool full_rows;     // the kind starts on the full-row Jacobi kernels (diffusion / reaction terms: no upwind rows)
};
struct SweepPlan {
    int budget, kbudget;    // what `step` enqueues: Jacobi sweeps and species-solve iterations per step
    bool meshp, cheb;       // one-workgroup step; Chebyshev species solve
};
enum { FEMFCT_SWEEP_REPEAT = -1 };  // verdict: neither accepted (FEMFCT_OK) nor failed (FEMFCT_ERR_*, all positive)
// sets ctx->pair_rows / ctx->solver for the attempt and picks its budgets from the kind's record
FEMFCT_INTERNAL int femfct_sweep_plan(femfct_ctx* ctx, const SweepSpec& sp, SweepPlan* plan);
// copies the step logs of the sweep just enqueued into h_log / h_klog and waits for them
FEMFCT_INTERNAL int femfct_sweep_fetch_logs(femfct_ctx* ctx, const SweepSpec& sp);
// reads the logs, updates the kind's record: FEMFCT_OK, FEMFCT_SWEEP_REPEAT or an error (femfct_fail)
FEMFCT_INTERNAL int femfct_sweep_verdict(femfct_ctx* ctx, const SweepSpec& sp, const SweepPlan& plan);
FEMFCT_INTERNAL void femfct_sweep_report_times(const SweepSpec& sp, const double t[4]);   // FEMFCT_DEBUG_TIMES=<ms>

// species-solve budget after a sweep whose worst step took `worst` iterations
// (Chebyshev reports the count that meets tol/10 at its asymptotic rate: no extra margin)
static inline int femfct_next_kry_budget(const femfct_ctx* ctx, int worst, bool cheb) {
    return std::min(ctx->kry_max_iters, cheb ? std::max(8, worst + 1) : std::max(8, worst + worst / 4 + 2));
}

// Replays `step(jacobi_budget, krylov_budget, reps)` until num_steps are done, then has the per-step solver logs
// inspected; if a sweep/iteration budget was too small anywhere the whole sweep is repeated with a
// larger one (the sweep's inputs are never overwritten, so a repeat is exact).
template <class Begin, class Step>
int femfct_run_sweep(femfct_ctx* ctx, const SweepSpec& sp, Begin&& begin, Step&& step) {
    struct RestoreSolver {       // the effective solver is per kind of sweep; the user's choice comes back on every exit
        femfct_ctx* c;
        ~RestoreSolver() { c->solver = c->solver_user; c->pair_rows = false; }
    } restore_solver{ctx};
    const bool dbg_t = getenv("FEMFCT_DEBUG_TIMES") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (;;) {
        SweepPlan plan;
        int rc = femfct_sweep_plan(ctx, sp, &plan);
        if (rc != FEMFCT_OK) return rc;
        double t[4] = {dbg_t ? now() : 0.0, 0.0, 0.0, 0.0};
        if ((rc = begin()) != FEMFCT_OK) return rc;
        if (dbg_t) t[1] = now();
        int32_t init[2] = {sp.level0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_level, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
        // several identical time steps per captured graph: fewer graph launches, no inter-graph gaps
        const int32_t per_graph = std::max(1, std::min(ctx->steps_per_graph, sp.num_steps));
        for (int32_t k = 0; k < sp.num_steps; k += per_graph) {
            rc = step(plan.budget, plan.kbudget, std::min(per_graph, sp.num_steps - k));
            if (rc != FEMFCT_OK) return rc;
        }
        if (dbg_t) t[2] = now();
        if ((rc = femfct_sweep_fetch_logs(ctx, sp)) != FEMFCT_OK) return rc;
        if (dbg_t) { t[3] = now(); femfct_sweep_report_times(sp, t); }
        rc = femfct_sweep_verdict(ctx, sp, plan);
        if (rc != FEMFCT_SWEEP_REPEAT) return rc;
    }
}
