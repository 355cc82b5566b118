// The snapshot-tracking entry points of the three PDE systems (femfct_nonlinear_adjoint_obs, femfct_schnak_adjoint_obs,
// femfct_chtxs_adjoint_obs) under AddressSanitizer on the fake HIP runtime: argument handling, workspace sizes and graph
// keys of the HOST code, with growing / shrinking batch and step counts, with and without a window, one variable
// unobserved (null theta, null target), both chemotaxis loads, with and without growth and a time-dependent wind,
// alternating with the existing adjoint sweeps on the same context (their graphs must not be taken for one another's), and
// with FEMFCT_FORM_GROUPS=0.  Kernels do not run.
#include "../../include/femfct.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define OK(x) do { int rc_ = (x); if (rc_ != FEMFCT_OK) { printf("line %d: rc %d (%s)\n", __LINE__, rc_, femfct_last_error(ctx)); fails++; } } while (0)
#define BAD(x) do { int rc_ = (x); if (rc_ != FEMFCT_ERR_INVALID) { printf("line %d: expected FEMFCT_ERR_INVALID, got %d\n", __LINE__, rc_); fails++; } } while (0)

static double* dmalloc(femfct_ctx* ctx, size_t count) {
    void* p = nullptr;
    if (femfct_malloc(ctx, &p, count * sizeof(double)) != FEMFCT_OK) abort();
    femfct_memset0(ctx, p, count * sizeof(double));
    return (double*)p;
}

static int run(int groups) {
    int fails = 0;
    setenv("FEMFCT_FORM_GROUPS", groups ? "1" : "0", 1);
    const double spar[6] = {0.01, 8.6676, 0.9, 230.82, 100.0, 0.6}, cpar[5] = {100.0, 0.05, 0.05, 0.25, 0.5};
    const double growth[3] = {0.0, 1.0, -1.0}, bad_growth[3] = {0.0, NAN, -1.0};
    for (int order = 0; order < 2; ++order)
        for (int nc : {4, 20, 45, 80}) {
            femfct_ctx* ctx = nullptr;
            if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
            OK(femfct_set_mesh_square(ctx, 0.0, 1.0, nc, order));
            const int n = (nc + 1) * (nc + 1), W = 7;
            double* Aw = dmalloc(ctx, (size_t)W * n);
            double* win = dmalloc(ctx, n);
            for (int pass = 0; pass < 3; ++pass) {
                const int Nt = pass == 1 ? 9 : 4, B = pass == 1 ? 5 : (pass == 2 ? 1 : 2);     // grow, then shrink
                const size_t tl = (size_t)(Nt + 1) * n;
                double *u = dmalloc(ctx, tl * B), *v = dmalloc(ctx, tl * B), *uh = dmalloc(ctx, tl * B), *vh = dmalloc(ctx, tl * B),
                       *p = dmalloc(ctx, tl * B), *q = dmalloc(ctx, tl * B), *c = dmalloc(ctx, tl * B), *thu = dmalloc(ctx, Nt + 1),
                       *thv = dmalloc(ctx, Nt + 1);
                std::vector<double> ws((size_t)Nt + 1, 0.5);
                for (const double* w : {(const double*)nullptr, (const double*)win}) {
                    OK(femfct_nonlinear_adjoint_obs(ctx, Aw, u, uh, thu, 1.0, w, p, Nt, 1e-3, 1e-4, B));
                    OK(femfct_nonlinear_adjoint_alltime(ctx, Aw, u, uh, 0, p, Nt, 1e-3, 1e-4, B));
                    OK(femfct_nonlinear_adjoint_obs(ctx, Aw, u, uh, thu, 0.0, w, p, Nt, 1e-3, 1e-4, B));
                    OK(femfct_nonlinear_adjoint_obs(ctx, Aw, u, nullptr, nullptr, 0.0, w, p, Nt, 1e-3, 1e-4, B));
                    OK(femfct_nonlinear_adjoint(ctx, Aw, u, uh, p, Nt, 1e-3, 1e-4, B));
                    for (const double* wsc : {(const double*)nullptr, (const double*)ws.data()}) {
                        OK(femfct_schnak_adjoint_obs(ctx, Aw, wsc, u, v, uh, vh, thu, 1.0, thv, 0.0, w, p, q, Nt, 5e-4, spar, B));
                        OK(femfct_schnak_adjoint_tw(ctx, Aw, wsc, u, v, uh, vh, p, q, Nt, 5e-4, spar, 1, B));
                        OK(femfct_schnak_adjoint_obs(ctx, Aw, wsc, u, v, uh, nullptr, thu, 0.5, nullptr, 0.0, w, p, q, Nt, 5e-4, spar, B));
                        OK(femfct_schnak_adjoint_obs(ctx, Aw, wsc, u, v, nullptr, vh, nullptr, 0.0, thv, 2.0, w, p, q, Nt, 5e-4, spar, B));
                    }
                    for (const double* g : {(const double*)nullptr, (const double*)growth})
                        for (int misfit : {FEMFCT_MISFIT_NODAL, FEMFCT_MISFIT_MASS}) {
                            OK(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, w, p, q, c, Nt, 5e-4, cpar, 0.1, g, misfit, B));
                            OK(femfct_chtxs_adjoint_g(ctx, u, v, uh, vh, p, q, c, Nt, 5e-4, cpar, 0.1, 1, g, B));
                            OK(femfct_chtxs_adjoint_obs(ctx, u, v, uh, nullptr, thu, 1.0, nullptr, 0.0, w, p, q, c, Nt, 5e-4, cpar, 0.1, g, misfit, B));
                            OK(femfct_chtxs_adjoint_obs(ctx, u, v, nullptr, vh, nullptr, 0.0, thv, 0.0, w, p, q, c, Nt, 5e-4, cpar, 0.1, g, misfit, B));
                        }
                }
                std::vector<femfct_step_info> info((size_t)Nt * B);
                OK(femfct_traj_info(ctx, info.data(), Nt, B));
                OK(femfct_traj_krylov_info(ctx, info.data(), Nt, B));
                BAD(femfct_nonlinear_adjoint_obs(ctx, Aw, u, uh, thu, NAN, nullptr, p, Nt, 1e-3, 1e-4, B));
                BAD(femfct_nonlinear_adjoint_obs(ctx, Aw, u, nullptr, thu, 1.0, nullptr, p, Nt, 1e-3, 1e-4, B));       // observed, no target
                BAD(femfct_nonlinear_adjoint_obs(ctx, Aw, u, uh, thu, 1.0, nullptr, nullptr, Nt, 1e-3, 1e-4, B));
                BAD(femfct_nonlinear_adjoint_obs(ctx, Aw, u, uh, thu, 1.0, nullptr, p, 0, 1e-3, 1e-4, B));
                BAD(femfct_schnak_adjoint_obs(ctx, Aw, nullptr, u, v, uh, vh, thu, INFINITY, thv, 0.0, nullptr, p, q, Nt, 5e-4, spar, B));
                BAD(femfct_schnak_adjoint_obs(ctx, Aw, nullptr, u, v, uh, vh, thu, 1.0, thv, NAN, nullptr, p, q, Nt, 5e-4, spar, B));
                BAD(femfct_schnak_adjoint_obs(ctx, Aw, nullptr, u, v, uh, nullptr, thu, 1.0, thv, 1.0, nullptr, p, q, Nt, 5e-4, spar, B));
                BAD(femfct_schnak_adjoint_obs(ctx, Aw, nullptr, u, v, uh, vh, thu, 1.0, thv, 1.0, nullptr, p, q, Nt, 5e-4, nullptr, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.1, nullptr, 2, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.1, nullptr, -1, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, NAN, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.1, nullptr, 1, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.1, bad_growth, 1, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, nullptr, vh, thu, 1.0, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.1, nullptr, 1, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, nullptr, p, q, nullptr, Nt, 5e-4, cpar, 0.1, nullptr, 1, B));
                BAD(femfct_chtxs_adjoint_obs(ctx, u, v, uh, vh, thu, 1.0, thv, 0.0, nullptr, p, q, c, Nt, 5e-4, cpar, 0.0, nullptr, 1, B));
                for (double* a : {u, v, uh, vh, p, q, c, thu, thv}) OK(femfct_free(ctx, a));
            }
            OK(femfct_set_graphs(ctx, 0));
            {
                double *u = dmalloc(ctx, 4 * (size_t)n), *p = dmalloc(ctx, 4 * (size_t)n), *q = dmalloc(ctx, 4 * (size_t)n), *th = dmalloc(ctx, 4);
                OK(femfct_nonlinear_adjoint_obs(ctx, Aw, u, u, th, 1.0, win, p, 3, 1e-3, 1e-4, 1));
                OK(femfct_schnak_adjoint_obs(ctx, Aw, nullptr, u, u, u, u, th, 1.0, th, 1.0, win, p, q, 3, 5e-4, spar, 1));
                OK(femfct_chtxs_adjoint_obs(ctx, u, u, u, u, th, 1.0, th, 1.0, win, p, q, u, 3, 5e-4, cpar, 0.1, growth, FEMFCT_MISFIT_MASS, 1));
                for (double* a : {u, p, q, th}) OK(femfct_free(ctx, a));
            }
            OK(femfct_free(ctx, Aw)); OK(femfct_free(ctx, win));
            OK(femfct_destroy(ctx));
        }
    return fails;
}

int main() {
    int fails = run(1) + run(0);
    if (femfct_chtxs_adjoint_obs(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, nullptr, 0.0, nullptr, nullptr, nullptr, nullptr,
                                 1, 1.0, nullptr, 0.1, nullptr, 1, 1) == FEMFCT_OK) { printf("null ctx accepted\n"); fails++; }
    printf("sysobs_asan_driver: %d unexpected return codes\n", fails);
    return fails ? 1 : 0;
}
