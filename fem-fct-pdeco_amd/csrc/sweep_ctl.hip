// The sweep controller: what femfct_run_sweep (traj_common.h) does between the drivers' begin / step lambdas.  Host code
// only.  Per attempt: plan (budgets and kernels from the kind's record) -> run -> fetch logs -> verdict (accept, repeat
// with another budget or solver, or fail).  The record is SweepKindState (femfct_internal.h).
#include "traj_common.h"

// ---- what the setters forget -------------------------------------------------------------------------------------
// Which memory of a kind survives which setter (x = reset to its starting value):
//                      budget  good  fail  mesh_cap  cheb_budget  bicg_budget  full_rows  low_bicg  cheb_off
//   femfct_set_solver     x      .     .      .          .            .           .          x         .
//   femfct_set_fusion     x      .     .      .          .            .           .          .         .
//   femfct_set_species_   .      .     .      .          .            .           .          .         x
//     solver
// Nothing else resets a record: they also outlive a change of mesh.  (good / fail / mesh_cap surviving a change of
// max_iters is known and left alone here: ADVICE.md item 2)
void femfct_forget_jacobi_budgets(femfct_ctx* ctx) {
    for (auto& k : ctx->kinds) k.second.budget = SweepKindState().budget;
}
void femfct_forget_bicgstab_handovers(femfct_ctx* ctx) {
    for (auto& k : ctx->kinds) k.second.low_bicg = false;
}
void femfct_forget_cheb_off(femfct_ctx* ctx) {
    for (auto& k : ctx->kinds) k.second.cheb_off = false;
}

int femfct_sweep_plan(femfct_ctx* ctx, const SweepSpec& sp, SweepPlan* plan) {
    SweepKindState& st = ctx->kinds[sp.kind];
    if (sp.full_rows) st.full_rows = true;
    // bandwidth regime: rows of an upwind operator as one value per opposing pair (k_strip_jacobi_pair_walk), until a
    // sweep of this kind shows a row that is not one (FEMFCT_FLAG_ROW_PAIRS, femfct_sweep_verdict)
    ctx->pair_rows = !st.full_rows;
    // a kind whose operator lies outside the scheme's dt restriction (Jacobi does not contract: the reference's
    // spsolve does not care, helpers.py:1782) is solved with Jacobi-preconditioned BiCGStab from then on
    ctx->solver = st.low_bicg ? FEMFCT_SOLVER_BICGSTAB : ctx->solver_user;
    if (ctx->solver == FEMFCT_SOLVER_BICGSTAB) {
        int rk = femfct_ensure_krylov_ws(ctx, sp.batch);
        if (rk != FEMFCT_OK) return rk;
    }
    // species solves: Chebyshev (structured mesh) and BiCGStab keep separate iteration budgets
    plan->cheb = sp.krylov && femfct_species_cheb(ctx, sp.kind);
    // the one-workgroup step (kernels_mesh.hip) stops by itself: its budget is only a cap, kept fixed so that every sweep
    // of the kind replays the same captured graphs (a budget that follows the iteration counts would re-capture them)
    plan->meshp = femfct_mesh_step_wanted(ctx, sp.batch);
    if (plan->meshp && !st.mesh_cap) st.mesh_cap = std::min(ctx->max_iters, 96);
    plan->budget = plan->meshp ? st.mesh_cap : femfct_round_budget(ctx, st.budget);
    plan->kbudget = femfct_round_kry_budget(ctx, plan->cheb ? st.cheb_budget : st.bicg_budget);
    return FEMFCT_OK;
}

int femfct_sweep_fetch_logs(femfct_ctx* ctx, const SweepSpec& sp) {
    ctx->log_steps = ctx->log_batch = 0;      // no matching log while the copies are in flight / after a failure
    ctx->h_log.resize((size_t)sp.num_steps * sp.batch);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_log.data(), ctx->d_log, sizeof(StepCtl) * ctx->h_log.size(), hipMemcpyDeviceToHost,
                                ctx->stream));
    if (sp.krylov) {
        ctx->h_klog.resize(sizeof(KrylovCtl) * (size_t)sp.num_steps * sp.batch);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_klog.data(), ctx->d_klog, ctx->h_klog.size(), hipMemcpyDeviceToHost, ctx->stream));
    } else {
        ctx->h_klog.clear();
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->log_steps = sp.num_steps;
    ctx->log_batch = sp.batch;
    return FEMFCT_OK;
}

void femfct_sweep_report_times(const SweepSpec& sp, const double t[4]) {
    if (t[3] - t[0] > atof(getenv("FEMFCT_DEBUG_TIMES")))      // FEMFCT_DEBUG_TIMES=<ms>: report sweeps that take longer
        fprintf(stderr, "[femfct] sweep kind %d took %.1f ms: begin %.2f, enqueue %.2f, wait %.2f\n", (int)sp.kind, t[3] - t[0],
                t[1] - t[0], t[2] - t[1], t[3] - t[2]);
}

namespace {

struct LogSummary {
    int worst = 0, kworst = 0;                  // most Jacobi sweeps / species-solve iterations of any step
    bool short_budget = false, kshort = false;  // some step ran out of its budget
    bool coarse = false;                        // `worst` counts whole launches
    double worst_res = 0.0, kworst_res = 0.0;   // largest residual among the steps that ran out (NaN counts as Inf: diverged)
};

bool any_row_pairs(const femfct_ctx* ctx) {
    bool not_pairs = false;
    for (const StepCtl& c : ctx->h_log) not_pairs = not_pairs || (c.flags & FEMFCT_FLAG_ROW_PAIRS);
    return not_pairs;
}

LogSummary summarise_logs(const femfct_ctx* ctx, const SweepSpec& sp) {
    LogSummary s;
    for (const StepCtl& c : ctx->h_log) {
        if (c.iters > s.worst) s.coarse = (c.flags & FEMFCT_FLAG_COARSE_ITERS) != 0;
        s.worst = std::max(s.worst, c.iters);
        if (c.flags & FEMFCT_FLAG_SOLVER_BUDGET) {
            s.short_budget = true;
            s.worst_res = (c.resid == c.resid) ? std::max(s.worst_res, c.resid) : INFINITY;
        }
    }
    if (sp.krylov) {
        const KrylovCtl* kl = (const KrylovCtl*)ctx->h_klog.data();
        for (size_t k = 0; k < (size_t)sp.num_steps * sp.batch; ++k) {
            s.kworst = std::max(s.kworst, kl[k].iters);
            if ((kl[k].flags & FEMFCT_FLAG_SOLVER_BUDGET) || !(kl[k].resid == kl[k].resid)) {
                s.kshort = true;
                s.kworst_res = std::max(s.kworst_res, kl[k].resid == kl[k].resid ? kl[k].resid : INFINITY);
            }
        }
    }
    return s;
}

// Jacobi budget of the kind's next sweep after one that `budget` sufficed for
int next_jacobi_budget(const femfct_ctx* ctx, const SweepKindState& st, int32_t batch, int budget, int worst, bool coarse) {
    // whole-mesh workgroups stop by themselves: the budget is only an upper bound, keep a margin
    if (femfct_tile4_wanted(ctx, batch) && femfct_single_patch(ctx, batch)) return std::min(ctx->max_iters, worst + 6);
    // Tiles report whole launches: `worst` = U launches of K sweeps, and every step was still above
    // the tolerance after (U-1)*K.  If one launch fewer of the deepest halo could cover that, try it
    // once (a failure is remembered per kind and costs one repeated sweep).
    int K = 0, U = 0, K2 = 0, U2 = 0;
    if (femfct_jacobi_plan(ctx, budget, batch, &K, &U) && worst > 0) {
        U = (worst + K - 1) / K;
        const int lb = (U - 1) * K;
        int top = 0;
        for (int b_try = lb + 1; U >= 2 && b_try < worst; ++b_try)
            if (femfct_jacobi_plan(ctx, b_try, batch, &K2, &U2) && U2 <= U - 1) top = b_try;
        if (top > lb && top > st.fail && 10 * top >= 7 * worst) return top;
    }
    return femfct_next_budget(ctx, worst, coarse);
}

}  // namespace

int femfct_sweep_verdict(femfct_ctx* ctx, const SweepSpec& sp, const SweepPlan& plan) {
    SweepKindState& st = ctx->kinds[sp.kind];
    const int kind = sp.kind, budget = plan.budget, kbudget = plan.kbudget;
    const bool dbg = getenv("FEMFCT_DEBUG") != nullptr;
    if (any_row_pairs(ctx)) {        // what the pair-compact launches computed is void: repeat with the full-row kernels
        if (dbg) fprintf(stderr, "[femfct] sweep kind %d: rows with both entries of a pair -> full-row Jacobi launches\n", kind);
        st.full_rows = true;
        ctx->log_steps = ctx->log_batch = 0;
        return FEMFCT_SWEEP_REPEAT;
    }
    LogSummary s = summarise_logs(ctx, sp);
    if (dbg)
        fprintf(stderr, "[femfct] sweep kind %d: budget %d (krylov %d) worst %d kworst %d short %d/%d, %d graphs captured so far (%zu cached)\n",
                kind, budget, kbudget, s.worst, s.kworst, (int)s.short_budget, (int)s.kshort, ctx->graph_captures, ctx->graphs.size());
    int& kry_budget = plan.cheb ? st.cheb_budget : st.bicg_budget;
    // the one-workgroup step ran into its cap while contracting: double the cap (it never shrinks)
    if (s.short_budget && plan.meshp && budget < ctx->max_iters && s.worst_res < 1.0) {
        st.mesh_cap = std::min(ctx->max_iters, 2 * budget);
        s.short_budget = false;
        if (!s.kshort) return FEMFCT_SWEEP_REPEAT;
    }
    if (!s.short_budget && !s.kshort) {     // accepted
        if (!plan.meshp) {                  // (the one-workgroup step keeps its cap: budget, good and fail stay as they are)
            st.good = budget;
            st.budget = next_jacobi_budget(ctx, st, sp.batch, budget, s.worst, s.coarse);
        }
        if (sp.krylov) kry_budget = femfct_next_kry_budget(ctx, s.kworst, plan.cheb);
        return FEMFCT_OK;
    }
    if (s.short_budget) {
        st.fail = std::max(st.fail, budget);
        // no contraction at all (residual not below ||b|| after a whole budget, or not a number), or the sweep cap
        // reached: hand this kind of sweep to BiCGStab and repeat it
        const bool hopeless = !(s.worst_res < 1.0) || budget >= ctx->max_iters;
        if (hopeless && ctx->solver == FEMFCT_SOLVER_JACOBI) {
            if (dbg)
                fprintf(stderr, "[femfct] sweep kind %d: Jacobi residual %.3e after %d sweeps -> BiCGStab\n", kind, s.worst_res, budget);
            st.low_bicg = true;
            st.budget = 40;
            st.fail = st.good = 0;
            femfct_drop_graphs(ctx);
            return FEMFCT_SWEEP_REPEAT;
        }
        // a residual that is not finite (NaN or Inf in the data) stays so whatever the budget: fail now
        if (budget >= ctx->max_iters || !(s.worst_res < INFINITY))
            return femfct_fail(ctx, FEMFCT_ERR_NOT_CONVERGED, "low-order solve: residual %.3e after %d %s (tol %.1e)",
                               s.worst_res, budget,
                               ctx->solver == FEMFCT_SOLVER_BICGSTAB ? "BiCGStab iterations" : "Jacobi sweeps", ctx->rel_tol);
        // a failed attempt at fewer launches goes back to the budget that worked
        st.budget = st.good > budget ? st.good : femfct_grow_budget(ctx, budget);
    }
    if (s.kshort && plan.cheb) {
        // not contracting (complex spectrum outside the assumed interval) or out of budget: BiCGStab
        if (!(s.kworst_res < 10.0) || kbudget >= ctx->kry_max_iters) st.cheb_off = true;
        else st.cheb_budget = std::min(ctx->kry_max_iters, std::max(kbudget + 10, s.kworst + s.kworst / 10 + 5));
    } else if (s.kshort) {
        if (kbudget >= ctx->kry_max_iters || !(s.kworst_res < INFINITY))
            return femfct_fail(ctx, FEMFCT_ERR_NOT_CONVERGED, "BiCGStab: residual %.3e after %d iterations (tol %.1e)",
                               s.kworst_res, kbudget, ctx->kry_tol);
        st.bicg_budget = std::min(ctx->kry_max_iters, kbudget * 2);
    }
    return FEMFCT_SWEEP_REPEAT;
}
