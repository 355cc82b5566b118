// Characterises the sweep controller (csrc/sweep_ctl.hip, femfct_run_sweep in csrc/traj_common.h) on a box without a GPU,
// on top of the fake HIP runtime (fake_hip.cpp).  The driver calls femfct_run_sweep directly with its own begin / step
// lambdas; `step` launches nothing and writes scripted StepCtl / KrylovCtl entries into ctx->d_log / ctx->d_klog the way the
// device would report a step that needs X sweeps / Y iterations.  One trace line per attempt (what `step` received and
// saw), the library's own FEMFCT_DEBUG lines merged in, the return code and error text of every sweep.  The trace is
// compared with tests/golden/sweep_ctl_trace.txt (tests/test_sweep_ctl_host.py), recorded from the commit before the
// controller was split up: the driver looks at the controller only through what `step` observes, never at its record.
#include "traj_common.h"

#include <math.h>
#include <unistd.h>

namespace {

int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != FEMFCT_OK) { printf("line %d: rc %d (%s)\n", __LINE__, rc_, femfct_last_error(ctx)); fails++; } } while (0)
#define CHECK(c) do { if (!(c)) { printf("line %d: check failed: %s\n", __LINE__, #c); fails++; } } while (0)

// what the scripted device needs per step
struct Script {
    int need = 10;              // Jacobi sweeps
    int need_bicg = 12;         // BiCGStab iterations once the low-order solve was handed over
    double resid = 1e-3;        // residual reported when the Jacobi budget runs out
    double resid_bicg = 1e-3;   // ... when the BiCGStab budget of the low-order solve runs out
    int kneed_cheb = 20, kneed_bicg = 25;           // species solve
    double kresid_cheb = 1e-3, kresid_bicg = 1e-3;
    bool row_pairs = false;     // the operator has rows with both entries of a pair (seen by the pair-compact launch only)
    int hard_step = -1;         // >= 0: only this step needs `need`, the others half of it
};

const char* regime_name(int r) {
    switch (r) {
        case FEMFCT_REGIME_ROWS: return "rows";
        case FEMFCT_REGIME_STRIPS: return "strips";
        case FEMFCT_REGIME_TILE32: return "tile32";
        case FEMFCT_REGIME_PATCH64: return "patch64";
        case FEMFCT_REGIME_MESH: return "mesh";
    }
    return "?";
}

int sweep(femfct_ctx* ctx, const char* label, SweepKind kind, int32_t num_steps, int32_t batch, bool krylov, bool full_rows,
          const Script& sc) {
    OK(femfct_ensure_traj_ws(ctx, batch, num_steps));
    if (krylov) OK(femfct_ensure_krylov_ws(ctx, batch));
    printf("sweep %s: kind %d, %d steps x %d, regime %s\n", label, (int)kind, num_steps, batch,
           regime_name(femfct_kernel_regime(ctx, batch)));
    int ord = 0, attempt = 0;
    auto begin = [&]() { ord = 0; return (int)FEMFCT_OK; };
    auto step = [&](int budget, int kbudget, int reps) {
        const bool cheb = femfct_species_cheb(ctx, kind);
        if (ord == 0) {
            printf("  attempt %d: budget %d kbudget %d reps %d | solver %d pair_rows %d cheb %d | graphs cached %zu\n", ++attempt,
                   budget, kbudget, reps, ctx->solver, (int)ctx->pair_rows, (int)cheb, ctx->graphs.size());
            // a stand-in for the sweep's captured graph, so that a femfct_drop_graphs shows in the next attempt's line
            if (ctx->graphs.empty()) ctx->graphs[femfct_ctx::GraphKey{0}] = (hipGraphExec_t)malloc(8);
        }
        int K = 0, U = 0;
        // tiles report whole launches; workgroups that hold the whole mesh stop by themselves and report the exact count
        const bool tiles = femfct_jacobi_plan(ctx, budget, batch, &K, &U) && !femfct_mesh_step_wanted(ctx, batch) &&
                           !(femfct_tile4_wanted(ctx, batch) && femfct_single_patch(ctx, batch));
        for (int r = 0; r < reps; ++r, ++ord)
            for (int b = 0; b < batch; ++b) {
                StepCtl c{};
                const bool bicg = ctx->solver == FEMFCT_SOLVER_BICGSTAB;
                int need = bicg ? sc.need_bicg : sc.need;
                if (sc.hard_step >= 0 && ord != sc.hard_step) need /= 2;
                if (need > budget) {
                    c.flags |= FEMFCT_FLAG_SOLVER_BUDGET;
                    c.iters = budget;
                    c.resid = bicg ? sc.resid_bicg : sc.resid;
                } else if (tiles && !bicg) {
                    c.iters = (need + K - 1) / K * K;
                    c.flags |= FEMFCT_FLAG_COARSE_ITERS;
                    c.done = 1;
                } else {
                    c.iters = need;
                    c.done = 1;
                }
                if (sc.row_pairs && ctx->pair_rows) c.flags |= FEMFCT_FLAG_ROW_PAIRS;
                c.bnorm = 1.0;
                ctx->d_log[(size_t)ord * batch + b] = c;
                if (!krylov) continue;
                KrylovCtl k{};
                const int kneed = cheb ? sc.kneed_cheb : sc.kneed_bicg;
                if (kneed > kbudget) {
                    k.flags |= FEMFCT_FLAG_SOLVER_BUDGET;
                    k.iters = kbudget;
                    k.resid = cheb ? sc.kresid_cheb : sc.kresid_bicg;
                } else {
                    k.iters = kneed;
                    k.done = 1;
                }
                if (cheb) k.flags |= FEMFCT_FLAG_CHEBYSHEV;
                k.bnorm = 1.0;
                ((KrylovCtl*)ctx->d_klog)[(size_t)ord * batch + b] = k;
            }
        return (int)FEMFCT_OK;
    };
    const int rc = femfct_run_sweep(ctx, SweepSpec{kind, num_steps, batch, 0, krylov, full_rows}, begin, step);
    printf("  -> rc %d%s%s | solver %d pair_rows %d\n", rc, rc ? ": " : "", rc ? femfct_last_error(ctx) : "", ctx->solver,
           (int)ctx->pair_rows);
    return rc;
}

femfct_ctx* make_ctx(int nc, int order, int32_t batch, int want_a, int want_b) {
    femfct_ctx* ctx = nullptr;
    if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); exit(1); }
    OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, order));
    const int r = femfct_kernel_regime(ctx, batch);
    printf("mesh %d x %d, order %d, batch %d: regime %s\n", nc + 1, nc + 1, order, batch, regime_name(r));
    CHECK(r == want_a || r == want_b);
    return ctx;
}

}  // namespace

int main() {
    setenv("FEMFCT_DEBUG", "1", 1);
    unsetenv("FEMFCT_DEBUG_TIMES");
    setvbuf(stdout, nullptr, _IONBF, 0);
    dup2(STDOUT_FILENO, STDERR_FILENO);      // the library's FEMFCT_DEBUG lines, in order
    const SweepKind FWD = SWEEP_SOLIDBODY_FORWARD, ADJ = SWEEP_SOLIDBODY_ADJOINT;
    const int T32 = FEMFCT_REGIME_TILE32, P64 = FEMFCT_REGIME_PATCH64, MESH = FEMFCT_REGIME_MESH;
    Script s;

    printf("== (a) (b) tile32: first sweep beyond 48 grows, is accepted, sets the next budget; an easier one shrinks it\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        s = Script(); s.need = 53;
        OK(sweep(ctx, "a1 hard", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "a2 hard again", FWD, 4, 1, false, false, s));
        s.need = 20;
        OK(sweep(ctx, "b1 easy", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "b2 easy again", FWD, 4, 1, false, false, s));
        s.need = 27; s.hard_step = 2;
        OK(sweep(ctx, "b3 one hard step", FWD, 4, 1, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (a) (b) strips: the budget grows by whole launches; rows (fusion off): it doubles, then follows the count with a margin\n");
    {
        femfct_ctx* ctx = make_ctx(40, FEMFCT_ORDER_FENICS, 2, FEMFCT_REGIME_STRIPS, FEMFCT_REGIME_ROWS);
        s = Script(); s.need = 70;
        OK(sweep(ctx, "a3 hard", FWD, 3, 2, false, false, s));
        s.need = 20;
        OK(sweep(ctx, "b4 easy", FWD, 3, 2, false, false, s));
        OK(sweep(ctx, "b5 easy again", FWD, 3, 2, false, false, s));
        OK(femfct_set_fusion(ctx, 0, 0));
        CHECK(femfct_kernel_regime(ctx, 2) == FEMFCT_REGIME_ROWS);
        s.need = 130;
        OK(sweep(ctx, "a4 hard, one sweep per launch", FWD, 3, 2, false, false, s));
        OK(sweep(ctx, "a5 hard again", FWD, 3, 2, false, false, s));
        s.need = 20;
        OK(sweep(ctx, "b6 easy", FWD, 3, 2, false, false, s));
        OK(sweep(ctx, "b7 easy again", FWD, 3, 2, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (c) one launch fewer: tried and failed (back to the good budget, not tried again), tried and succeeded\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        for (int need : {36, 36, 36, 36, 41, 41}) {
            s = Script(); s.need = need;
            char label[32];
            snprintf(label, sizeof label, "c need %d", need);
            OK(sweep(ctx, label, ADJ, 4, 1, false, false, s));
        }
        s = Script(); s.need = 25;
        for (int it = 0; it < 3; ++it) OK(sweep(ctx, "c need 25, another kind", SWEEP_NONLINEAR_ADJOINT, 4, 1, false, true, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (d) max_iters between easy and hard: the kind goes to BiCGStab; back at 400 it recovers\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        s = Script(); s.need = 20;
        OK(sweep(ctx, "d1 easy", FWD, 4, 1, false, false, s));
        OK(femfct_set_solver(ctx, FEMFCT_SOLVER_JACOBI, 1e-13, 30));
        OK(sweep(ctx, "d2 easy, cap 30", FWD, 4, 1, false, false, s));
        s.need = 53;
        OK(sweep(ctx, "d3 hard, cap 30", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "d4 hard again", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "d5 other kind, hard, cap 30, BiCGStab short too", ADJ, 4, 1, false, false, [&] { Script t = s; t.need_bicg = 35; return t; }()) ==
           FEMFCT_ERR_NOT_CONVERGED ? FEMFCT_OK : FEMFCT_ERR_INVALID);
        OK(femfct_set_solver(ctx, FEMFCT_SOLVER_JACOBI, 1e-13, 400));
        OK(sweep(ctx, "d6 hard, cap 400", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "d7 hard again", FWD, 4, 1, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (e) NaN / Inf residuals: Jacobi hands over to BiCGStab, BiCGStab fails the sweep\n");
    for (double bad : {(double)NAN, (double)INFINITY}) {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        s = Script(); s.need = 1000; s.need_bicg = 1000; s.resid = bad; s.resid_bicg = bad;
        CHECK(sweep(ctx, "e1 not finite", FWD, 4, 1, false, false, s) == FEMFCT_ERR_NOT_CONVERGED);
        CHECK(sweep(ctx, "e2 not finite again", FWD, 4, 1, false, false, s) == FEMFCT_ERR_NOT_CONVERGED);
        s = Script(); s.need = 1000; s.resid = 2.0;     // finite but not contracting: handed over, BiCGStab copes
        OK(sweep(ctx, "e3 no contraction", ADJ, 4, 1, false, false, s));
        // a species solve whose residual is not a number
        s = Script(); s.kneed_cheb = s.kneed_bicg = 100000; s.kresid_cheb = s.kresid_bicg = bad;
        CHECK(sweep(ctx, "e4 species solve not finite", SWEEP_SCHNAK_FORWARD, 4, 1, true, true, s) == FEMFCT_ERR_NOT_CONVERGED);
        OK(femfct_destroy(ctx));
    }
    printf("== (f) patch64: ROW_PAIRS repeats on full rows and stays there; diffusive and system kinds start there\n");
    {
        femfct_ctx* ctx = make_ctx(330, FEMFCT_ORDER_VERTEX, 1, P64, P64);
        s = Script(); s.need = 30;
        OK(sweep(ctx, "f1 upwind rows", FWD, 2, 1, false, false, s));
        s.row_pairs = true;
        OK(sweep(ctx, "f2 rows with pairs", FWD, 2, 1, false, false, s));
        OK(sweep(ctx, "f3 again", FWD, 2, 1, false, false, s));
        s.row_pairs = false;
        OK(sweep(ctx, "f4 upwind rows again: stays on full rows", FWD, 2, 1, false, false, s));
        s.row_pairs = true;
        OK(sweep(ctx, "f5 diffusive adjoint", ADJ, 2, 1, false, true, s));
        OK(sweep(ctx, "f6 the adjoint without diffusion afterwards", ADJ, 2, 1, false, false, s));
        OK(sweep(ctx, "f7 system kind", SWEEP_NONLINEAR_FORWARD, 2, 1, false, true, s));
        s = Script(); s.need = 37;
        OK(sweep(ctx, "f8 hard", FWD, 2, 1, false, false, s));
        OK(sweep(ctx, "f9 hard again", FWD, 2, 1, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (g) mesh regime: cap 96, doubled when a contracting step needs more, never shrinks; the Jacobi budget is left alone\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        s = Script(); s.need = 53;
        OK(sweep(ctx, "g1 tile32 first: budget, good and fail get values", FWD, 4, 1, false, false, s));
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, 40, FEMFCT_ORDER_VERTEX));
        CHECK(femfct_kernel_regime(ctx, 1) == MESH);
        s.need = 20;
        OK(sweep(ctx, "g2 easy", FWD, 4, 1, false, false, s));
        s.need = 120;
        OK(sweep(ctx, "g3 beyond the cap", FWD, 4, 1, false, false, s));
        s.need = 20;
        OK(sweep(ctx, "g4 easy: the cap stays", FWD, 4, 1, false, false, s));
        s.need = 500; s.need_bicg = 30;
        OK(sweep(ctx, "g5 beyond max_iters: BiCGStab", ADJ, 4, 1, false, false, s));
        s = Script(); s.need = 20; s.kneed_cheb = 60;
        OK(sweep(ctx, "g6 system kind, species budget short", SWEEP_SCHNAK_FORWARD, 4, 1, true, true, s));
        OK(sweep(ctx, "g7 again", SWEEP_SCHNAK_FORWARD, 4, 1, true, true, s));
        s.need = 120;
        OK(sweep(ctx, "g8 both short", SWEEP_SCHNAK_ADJOINT, 4, 1, true, true, s));
        OK(femfct_set_solver(ctx, FEMFCT_SOLVER_JACOBI, 1e-13, 100));
        s = Script(); s.need = 20;
        OK(sweep(ctx, "g9 max_iters 100: the cap of 192 is stale", FWD, 4, 1, false, false, s));
        OK(sweep(ctx, "g10 a kind first seen now", SWEEP_NONLINEAR_FORWARD, 4, 1, false, true, s));
        OK(femfct_set_solver(ctx, FEMFCT_SOLVER_JACOBI, 1e-13, 400));
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, 64, FEMFCT_ORDER_VERTEX));
        CHECK(femfct_kernel_regime(ctx, 1) == T32);
        s.need = 53;
        OK(sweep(ctx, "g11 tile32 again: what the mesh-regime sweeps left of good / fail", FWD, 4, 1, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (h) species solves: Chebyshev budget grows, Chebyshev is switched off, BiCGStab doubles, fails at the cap, comes back\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        const SweepKind K = SWEEP_SCHNAK_FORWARD;
        s = Script(); s.need = 20; s.kneed_cheb = 75;
        OK(sweep(ctx, "h1 Chebyshev needs 75", K, 4, 1, true, true, s));
        OK(sweep(ctx, "h2 again", K, 4, 1, true, true, s));
        s.kneed_cheb = 30;
        OK(sweep(ctx, "h3 easier", K, 4, 1, true, true, s));
        s.kneed_cheb = 200; s.kresid_cheb = 20.0; s.kneed_bicg = 100;
        OK(sweep(ctx, "h4 Chebyshev does not contract", K, 4, 1, true, true, s));
        OK(sweep(ctx, "h5 again: BiCGStab's own budget", K, 4, 1, true, true, s));
        OK(femfct_set_krylov(ctx, 1e-13, 120));
        s.kneed_bicg = 150;
        CHECK(sweep(ctx, "h6 BiCGStab beyond the cap of 120", K, 4, 1, true, true, s) == FEMFCT_ERR_NOT_CONVERGED);
        OK(femfct_set_species_solver(ctx, FEMFCT_SPECIES_AUTO));
        s.kresid_cheb = 1e-3; s.kneed_cheb = 150;
        OK(sweep(ctx, "h7 Chebyshev back, runs into the cap: off again", K, 4, 1, true, true, [&] { Script t = s; t.kneed_bicg = 90; return t; }()));
        OK(femfct_set_species_solver(ctx, FEMFCT_SPECIES_BICGSTAB));
        s.kneed_bicg = 60;
        OK(sweep(ctx, "h8 BiCGStab by choice", SWEEP_CHTXS_FORWARD, 4, 1, true, true, s));
        OK(femfct_destroy(ctx));
    }
    printf("== (i) two kinds interleaved\n");
    {
        femfct_ctx* ctx = make_ctx(64, FEMFCT_ORDER_VERTEX, 1, T32, T32);
        Script easy, hard;
        easy.need = 14; hard.need = 53;
        for (int it = 0; it < 3; ++it) {
            OK(sweep(ctx, "i forward, easy", FWD, 4, 1, false, false, easy));
            OK(sweep(ctx, "i adjoint, hard", ADJ, 4, 1, false, false, hard));
        }
        OK(femfct_destroy(ctx));
    }
    printf("== (j) what each setter makes the controller forget\n");
    {
        femfct_ctx* ctx = make_ctx(330, FEMFCT_ORDER_VERTEX, 1, P64, P64);
        // memories: forward on full rows with good / fail / budget; adjoint handed to BiCGStab; Schnakenberg with Chebyshev
        // off and grown species budgets
        Script f, a, k;
        f.need = 53; f.row_pairs = true;
        a.need = 1000; a.resid = 2.0; a.need_bicg = 30;
        k.need = 30; k.kneed_cheb = 200; k.kresid_cheb = 20.0; k.kneed_bicg = 100;
        auto all = [&](const char* when) {
            printf("-- %s\n", when);
            OK(sweep(ctx, "j forward", FWD, 2, 1, false, false, f));
            OK(sweep(ctx, "j adjoint", ADJ, 2, 1, false, false, a));
            OK(sweep(ctx, "j schnak", SWEEP_SCHNAK_FORWARD, 2, 1, true, true, k));
        };
        all("first sweeps");
        all("second sweeps");
        OK(femfct_set_fusion(ctx, 1, 1));
        all("after femfct_set_fusion");
        all("and again");
        OK(femfct_set_species_solver(ctx, FEMFCT_SPECIES_AUTO));
        all("after femfct_set_species_solver");
        all("and again");
        OK(femfct_set_solver(ctx, FEMFCT_SOLVER_JACOBI, 1e-13, 400));
        all("after femfct_set_solver");
        all("and again");
        OK(femfct_destroy(ctx));
    }
    printf("== (k) one patch covers the mesh: margin worst + 6\n");
    {
        femfct_ctx* ctx = make_ctx(44, FEMFCT_ORDER_VERTEX, 45, P64, P64);
        CHECK(femfct_tile4_wanted(ctx, 45) && femfct_single_patch(ctx, 45));
        s = Script(); s.need = 53;
        OK(sweep(ctx, "k1 hard", FWD, 2, 45, false, false, s));
        OK(sweep(ctx, "k2 hard again", FWD, 2, 45, false, false, s));
        s.need = 20;
        OK(sweep(ctx, "k3 easy", FWD, 2, 45, false, false, s));
        OK(sweep(ctx, "k4 easy again", FWD, 2, 45, false, false, s));
        OK(femfct_destroy(ctx));
    }
    printf("sweep_ctl_driver: %d unexpected results\n", fails);
    return fails ? 1 : 0;
}
