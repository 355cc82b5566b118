// The lockstep entry points (femfct_trial_controls, femfct_member_costs) under AddressSanitizer on the fake HIP runtime:
// every argument check, P*K at both limits, the levels x members > 65535 shape (scratch sizing, launch geometry), NULL
// cref and dist_host, shared and per-problem targets, both modes, alternating with the entry points that share the
// reduction scratch.  Kernels do not run.
#include "../../include/femfct.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define OK(x) do { int rc_ = (x); if (rc_ != FEMFCT_OK) { printf("line %d: rc %d (%s)\n", __LINE__, rc_, femfct_last_error(ctx)); fails++; } } while (0)
#define BAD(x) do { int rc_ = (x); if (rc_ != FEMFCT_ERR_INVALID) { printf("line %d: rc %d, expected FEMFCT_ERR_INVALID\n", __LINE__, rc_); fails++; } } while (0)

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
            const int n = (nc + 1) * (nc + 1);
            // (P, K, Nt): one member, a small batch, both limits of P*K, then a smaller one again (the scratch shrinks)
            const int shapes[][3] = {{1, 1, 4}, {3, 4, 6}, {256, 1, 2}, {1, 256, 2}, {16, 16, 1}, {2, 3, 5}};
            for (const auto& sh : shapes) {
                const int P = sh[0], K = sh[1], Nt = sh[2], members = P * K;
                const size_t tl = (size_t)(Nt + 1) * n;
                double *u = dmalloc(ctx, tl * members), *c = dmalloc(ctx, tl * members), *cout = dmalloc(ctx, tl * members),
                       *uh = dmalloc(ctx, tl * P), *cref = dmalloc(ctx, tl * P), *d = dmalloc(ctx, tl * P);
                // exactly P*K steps and P betas on the heap: a read past either trips the sanitizer
                std::vector<double> steps(members, 0.5), beta(P, 0.1), J(members, -1.0), dist(members, -1.0);
                OK(femfct_trial_controls(ctx, cref, d, steps.data(), P, K, 0.0, 5.0, (int64_t)tl, cout));
                OK(femfct_trial_controls(ctx, cref, d, steps.data(), P, K, 0.0, 5.0, 0, cout));
                for (int ft = 0; ft < 2; ++ft)
                    for (int per = 0; per < 2; ++per) {
                        OK(femfct_member_costs(ctx, u, uh, per, c, cref, beta.data(), P, K, Nt, 1e-3, ft, J.data(), dist.data()));
                        OK(femfct_member_costs(ctx, u, uh, per, c, nullptr, beta.data(), P, K, Nt, 1e-3, ft, J.data(), nullptr));
                        OK(femfct_member_costs(ctx, u, uh, per, c, nullptr, beta.data(), P, K, Nt, 1e-3, ft, J.data(), dist.data()));
                    }
                if (members <= 64) {      // the entry points that share the scratch, between two lockstep calls
                    OK(femfct_cost_functional(ctx, u, u, c, 0, Nt, 1e-3, 0.1, 0, nullptr, nullptr, J.data(), members));
                    OK(femfct_l2_norm_sq_Q(ctx, c, nullptr, Nt, 1e-3, dist.data(), members));
                    OK(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                }
                // argument checks
                BAD(femfct_trial_controls(ctx, nullptr, d, steps.data(), P, K, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, nullptr, steps.data(), P, K, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, nullptr, P, K, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), P, K, 0.0, 5.0, (int64_t)tl, nullptr));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), P, K, 0.0, 5.0, -1, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), 0, K, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), P, 0, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), -P, -K, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), 257, 1, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), 1, 257, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_trial_controls(ctx, cref, d, steps.data(), 65536, 65536, 0.0, 5.0, (int64_t)tl, cout));
                BAD(femfct_member_costs(ctx, nullptr, uh, 0, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, nullptr, 0, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, nullptr, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, nullptr, P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), P, K, Nt, 1e-3, 0, nullptr, dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), nullptr));
                BAD(femfct_member_costs(ctx, u, uh, 2, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, -1, c, cref, beta.data(), P, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), 0, K, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), P, 0, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), 257, 1, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), 1, 257, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), 65536, 65536, Nt, 1e-3, 0, J.data(), dist.data()));
                BAD(femfct_member_costs(ctx, u, uh, 0, c, cref, beta.data(), P, K, 0, 1e-3, 0, J.data(), dist.data()));
                for (double* a : {u, c, cout, uh, cref, d}) OK(femfct_free(ctx, a));
            }
            if (nc == 4) {      // levels x members = 701 x 96 = 67296 > 65535: beyond what the existing entry points take
                const int P = 12, K = 8, Nt = 700, members = P * K;
                const size_t tl = (size_t)(Nt + 1) * n;
                double *u = dmalloc(ctx, tl * members), *c = dmalloc(ctx, tl * members), *uh = dmalloc(ctx, tl * P),
                       *cref = dmalloc(ctx, tl * P);
                std::vector<double> beta(P, 0.1), J(members, -1.0), dist(members, -1.0);
                for (int ft = 0; ft < 2; ++ft)
                    OK(femfct_member_costs(ctx, u, uh, 1, c, cref, beta.data(), P, K, Nt, 1e-3, ft, J.data(), dist.data()));
                BAD(femfct_cost_functional(ctx, u, u, c, 0, Nt, 1e-3, 0.1, 0, nullptr, nullptr, J.data(), members));
                for (double* a : {u, c, uh, cref}) OK(femfct_free(ctx, a));
            }
            OK(femfct_destroy(ctx));
        }
    {   // no mass matrix registered, no context
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        double x[4] = {0, 0, 0, 0};
        BAD(femfct_member_costs(ctx, x, x, 0, x, nullptr, x, 1, 1, 1, 1e-3, 0, x, nullptr));
        OK(femfct_destroy(ctx));
        BAD(femfct_member_costs(nullptr, x, x, 0, x, nullptr, x, 1, 1, 1, 1e-3, 0, x, nullptr));
        BAD(femfct_trial_controls(nullptr, x, x, x, 1, 1, 0.0, 1.0, 4, x));
    }
    printf("lockstep_asan_driver: %d unexpected return codes\n", fails);
    return fails ? 1 : 0;
}
