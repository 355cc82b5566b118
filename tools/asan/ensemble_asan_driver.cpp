// femfct_ensemble_drift_gradient_rhs / femfct_ensemble_costs under AddressSanitizer on the fake HIP runtime: the host code
// that checks the arguments, lists the scenarios of non-zero weight into the by-value table, sizes the partials' scratch
// and the launches and copies the S + 2 results back, for S = 1 .. 256, a zero weight, cref present and absent, a window,
// level counts that make the scratch grow and then fit, and every argument check.  The result arrays live on the heap with
// exactly S entries: a write past them trips the sanitizer.  Kernels do not run (the results hold what the fake copy
// returns; only their extent is exercised).
#include "../../include/femfct.h"
#include <math.h>
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
    for (int nc : {4, 20, 300}) {                      // 300: n > 65536, four waves per block
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, 0));
        const int n = (nc + 1) * (nc + 1);
        for (int Nt : {1, 40, 7, 250, 3}) {            // the scratch grows (40, 250) and then fits (7, 3)
            if (nc == 300 && Nt > 7) continue;
            const int levels = Nt + 1;
            const size_t tl = (size_t)levels * n;
            const int Smax = nc == 300 ? 3 : 256;
            double *c = dmalloc(ctx, tl), *cref = dmalloc(ctx, tl), *out = dmalloc(ctx, tl), *cw = dmalloc(ctx, levels);
            double *win = dmalloc(ctx, n), *u = dmalloc(ctx, Smax * tl), *p = dmalloc(ctx, Smax * tl);
            for (int S : {1, 256, 2, 3, 64}) {
                if (S > Smax) continue;
                std::vector<double> w((size_t)S, 1.0 / S), T((size_t)S, -1.0), J(1, -1.0), dist(1, -1.0);
                OK(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w.data(), S, 1e-3, 1.0, 1.0, out, levels));
                OK(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w.data(), S, 1e-3, Nt, 0.01, T.data(), J.data(), dist.data()));
                OK(femfct_ensemble_costs(ctx, u, p, cw, win, c, nullptr, w.data(), S, 1e-3, Nt, 0.01, T.data(), J.data(), nullptr));
                if (S > 1) {                            // a zero weight, first and last
                    w[0] = 0.0;
                    OK(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w.data(), S, 1e-3, 1.0, 1.0, out, levels));
                    OK(femfct_ensemble_costs(ctx, u, p, cw, win, c, cref, w.data(), S, 0.0, Nt, 0.01, T.data(), J.data(), dist.data()));
                    w[0] = 1.0; w[S - 1] = 0.0;
                    OK(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w.data(), S, 1e-3, 1.0, 1.0, out, levels));
                    OK(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, nullptr, w.data(), S, 0.0, Nt, 0.01, T.data(), J.data(), nullptr));
                }
            }
            double w2[2] = {0.5, 0.5}, T[2], J[1], dist[1];
            std::vector<double> w257(257, 1.0);
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, nullptr, u, p, w2, 2, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, nullptr, p, w2, 2, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, nullptr, w2, 2, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, nullptr, 2, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w2, 2, 1e-3, 1.0, 1.0, nullptr, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w2, 0, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w257.data(), 257, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w2, 2, 1e-3, 1.0, 1.0, out, 0));
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w2, 2, 1e-3, 1.0, 1.0, out, 65536));
            BAD(femfct_ensemble_costs(ctx, nullptr, p, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, nullptr, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, nullptr, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, nullptr, cref, w2, 2, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, nullptr, 2, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, nullptr, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, nullptr, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, J, nullptr));   // cref without dist
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, nullptr, w2, 2, 1e-3, Nt, 0.01, T, J, dist));   // dist without cref
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 0, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w257.data(), 257, 1e-3, Nt, 0.01, T, J, dist));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 2, 1e-3, 0, 0.01, T, J, dist));
            for (double bad : {-1e-300, (double)NAN, (double)INFINITY}) {
                double wb[2] = {1.0, bad};
                BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, wb, 2, 1e-3, 1.0, 1.0, out, levels));
                BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, wb, 2, 1e-3, Nt, 0.01, T, J, dist));
            }
            double wz[2] = {0.0, 0.0};
            BAD(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, wz, 2, 1e-3, 1.0, 1.0, out, levels));
            BAD(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, wz, 2, 1e-3, Nt, 0.01, T, J, dist));
            OK(femfct_ensemble_costs(ctx, u, p, cw, nullptr, c, cref, w2, 2, 1e-3, Nt, 0.01, T, J, dist));       // still usable
            OK(femfct_ensemble_drift_gradient_rhs(ctx, c, u, p, w2, 2, 1e-3, 1.0, 1.0, out, levels));
            for (void* q : {(void*)c, (void*)cref, (void*)out, (void*)cw, (void*)win, (void*)u, (void*)p}) femfct_free(ctx, q);
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[2], w1[1] = {1.0}, T[1], J[1];
        BAD(femfct_ensemble_drift_gradient_rhs(ctx, xx, xx, xx, w1, 1, 1.0, 1.0, 1.0, xx, 1));     // no structured mesh
        BAD(femfct_ensemble_costs(ctx, xx, xx, xx, nullptr, xx, nullptr, w1, 1, 1.0, 1, 1.0, T, J, nullptr));
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_ensemble_drift_gradient_rhs(ctx, xx, xx, xx, w1, 1, 1.0, 1.0, 1.0, xx, 1));     // a pattern, still no mesh
        BAD(femfct_ensemble_costs(ctx, xx, xx, xx, nullptr, xx, nullptr, w1, 1, 1.0, 1, 1.0, T, J, nullptr));
        femfct_destroy(ctx);
        if (femfct_ensemble_drift_gradient_rhs(nullptr, xx, xx, xx, w1, 1, 1.0, 1.0, 1.0, xx, 1) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_ensemble_costs(nullptr, xx, xx, xx, nullptr, xx, nullptr, w1, 1, 1.0, 1, 1.0, T, J, nullptr) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("ensemble_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
