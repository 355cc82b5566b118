// The snapshot-tracking entry points (femfct_solidbody_adjoint_obs, femfct_linear_adjoint_react_obs, femfct_obs_load,
// femfct_obs_cost) under AddressSanitizer on the fake HIP runtime: argument handling, workspace sizes and graph keys of
// the HOST code, with growing / shrinking batch and step counts, with and without a window, alternating with the
// existing adjoint sweeps on the same context (their graphs must not be taken for one another's).  Kernels do not run.
#include "../../include/femfct.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define OK(x) do { int rc_ = (x); if (rc_ != FEMFCT_OK) { printf("line %d: rc %d (%s)\n", __LINE__, rc_, femfct_last_error(ctx)); fails++; } } while (0)
#define BAD(x) do { int rc_ = (x); if (rc_ == FEMFCT_OK) { printf("line %d: expected an error\n", __LINE__); fails++; } } while (0)

static double* dmalloc(femfct_ctx* ctx, size_t count) {
    void* p = nullptr;
    if (femfct_malloc(ctx, &p, count * sizeof(double)) != FEMFCT_OK) abort();
    femfct_memset0(ctx, p, count * sizeof(double));
    return (double*)p;
}

int main() {
    int fails = 0;
    for (int order = 0; order < 2; ++order)
        for (int nc : {4, 20, 80}) {
            femfct_ctx* ctx = nullptr;
            if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
            OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, order));
            const int n = (nc + 1) * (nc + 1), W = 7;
            double* Arot = dmalloc(ctx, (size_t)W * n);
            double* win = dmalloc(ctx, n);
            for (int pass = 0; pass < 3; ++pass) {
                const int Nt = pass == 1 ? 9 : 4, B = pass == 1 ? 5 : (pass == 2 ? 1 : 2);     // grow, then shrink
                const size_t tl = (size_t)(Nt + 1) * n;
                double *c = dmalloc(ctx, tl * B), *u = dmalloc(ctx, tl * B), *uh = dmalloc(ctx, tl * B), *p = dmalloc(ctx, tl * B),
                       *g = dmalloc(ctx, tl), *theta = dmalloc(ctx, Nt + 1), *cw = dmalloc(ctx, Nt + 1), *out = dmalloc(ctx, (size_t)n * B);
                std::vector<double> J(B, -1.0);
                for (const double* w : {(const double*)nullptr, (const double*)win}) {
                    OK(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, uh, theta, 1.0, w, p, Nt, 1e-3, 0.0, 1.0, 1.0, 1.0, B));
                    OK(femfct_solidbody_adjoint(ctx, Arot, c, 0, u, uh, p, Nt, 1e-3, 0.0, 1.0, 1.0, 1.0, 1, B));
                    OK(femfct_solidbody_adjoint_obs(ctx, Arot, c, 1, u, uh, theta, 0.0, w, p, Nt, 1e-3, 1e-3, 1.0, 1.0, 1.0, B));
                    OK(femfct_linear_adjoint_react_obs(ctx, Arot, g, u, uh, theta, 0.5, w, p, Nt, 1e-3, 1e-3, B));
                    OK(femfct_linear_adjoint_react(ctx, Arot, g, u, uh, p, Nt, 1e-3, 1e-3, 1, B));
                    OK(femfct_obs_load(ctx, u, uh, theta, Nt, 1e-3, w, out, B));
                    OK(femfct_obs_cost(ctx, u, uh, cw, w, Nt, B, J.data()));
                }
                std::vector<femfct_step_info> info((size_t)Nt * B);
                OK(femfct_traj_info(ctx, info.data(), Nt, B));
                BAD(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, uh, nullptr, 1.0, nullptr, p, Nt, 1e-3, 0.0, 1.0, 1.0, 1.0, B));
                BAD(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, uh, theta, -1.0, nullptr, p, Nt, 1e-3, 0.0, 1.0, 1.0, 1.0, B));
                BAD(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, nullptr, theta, 1.0, nullptr, p, Nt, 1e-3, 0.0, 1.0, 1.0, 1.0, B));
                BAD(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, uh, theta, 1.0, nullptr, p, 0, 1e-3, 0.0, 1.0, 1.0, 1.0, B));
                BAD(femfct_linear_adjoint_react_obs(ctx, Arot, g, u, uh, nullptr, 0.5, nullptr, p, Nt, 1e-3, 1e-3, B));
                BAD(femfct_linear_adjoint_react_obs(ctx, Arot, nullptr, u, uh, theta, 0.5, nullptr, p, Nt, 1e-3, 1e-3, B));
                BAD(femfct_obs_load(ctx, u, uh, nullptr, 0, 1e-3, nullptr, out, B));
                BAD(femfct_obs_load(ctx, u, uh, theta, -1, 1e-3, nullptr, out, B));
                BAD(femfct_obs_load(ctx, u, uh, theta, 0, 0.0, nullptr, out, B));
                BAD(femfct_obs_cost(ctx, u, uh, nullptr, nullptr, Nt, B, J.data()));
                BAD(femfct_obs_cost(ctx, u, uh, cw, nullptr, Nt, 0, J.data()));
                BAD(femfct_obs_cost(ctx, u, uh, cw, nullptr, Nt, B, nullptr));
                for (double* a : {c, u, uh, p, g, theta, cw, out}) OK(femfct_free(ctx, a));
            }
            OK(femfct_set_graphs(ctx, 0));
            {
                double *c = dmalloc(ctx, 4 * (size_t)n), *u = dmalloc(ctx, 4 * (size_t)n), *theta = dmalloc(ctx, 4);
                OK(femfct_solidbody_adjoint_obs(ctx, Arot, c, 0, u, u, theta, 1.0, win, c, 3, 1e-3, 0.0, 1.0, 1.0, 1.0, 1));
                for (double* a : {c, u, theta}) OK(femfct_free(ctx, a));
            }
            OK(femfct_free(ctx, Arot)); OK(femfct_free(ctx, win));
            OK(femfct_destroy(ctx));
        }
    BAD(femfct_obs_cost(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr));
    printf("obs_asan_driver: %d unexpected return codes\n", fails);
    return fails ? 1 : 0;
}
