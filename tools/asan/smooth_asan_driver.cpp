// femfct_smooth_cost / femfct_smooth_rhs / femfct_drift_gradient_rhs_smooth under AddressSanitizer on the fake HIP runtime:
// the host code that checks the arguments, sizes the partials' scratch and the launches, and copies the 2 * batch results
// back and interleaves them, for batch 1 and many, level counts that make the scratch grow and then fit, more than 65535
// (member, level) items, and every argument check.  The result arrays live on the heap with exactly 2 * batch entries: a
// write past them trips the sanitizer.  Kernels do not run (the results hold what the fake copy returns; only their extent
// is exercised).
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
            const int Bmax = nc == 4 ? 300 : (nc == 300 ? 2 : 16);     // nc = 4: 300 * 251 > 65535 items
            double *c = dmalloc(ctx, Bmax * tl), *out = dmalloc(ctx, Bmax * tl), *u = dmalloc(ctx, tl), *p = dmalloc(ctx, tl);
            for (int B : {1, 300, 2, 16, 3}) {
                if (B > Bmax) continue;
                std::vector<double> R(2 * (size_t)B, -1.0);
                OK(femfct_smooth_cost(ctx, c, Nt, 0.01, R.data(), B));
                OK(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, 0.01, out, B));
                OK(femfct_smooth_rhs(ctx, c, 0.0, 1e-6, Nt, 0.01, out, B));
                OK(femfct_smooth_rhs(ctx, c, 1e-3, 0.0, Nt, 0.01, out, B));
                OK(femfct_smooth_rhs(ctx, c, 0.0, 0.0, Nt, 0.01, out, B));
            }
            OK(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.01, out, levels, 1.0, 1.0));
            OK(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 0.0, 0.0, 0.01, out, levels, 1.0, 1.0));
            double R[2];
            BAD(femfct_smooth_cost(ctx, nullptr, Nt, 0.01, R, 1));
            BAD(femfct_smooth_cost(ctx, c, Nt, 0.01, nullptr, 1));
            BAD(femfct_smooth_cost(ctx, c, 0, 0.01, R, 1));
            BAD(femfct_smooth_cost(ctx, c, -3, 0.01, R, 1));
            BAD(femfct_smooth_cost(ctx, c, Nt, 0.01, R, 0));
            BAD(femfct_smooth_cost(ctx, c, Nt, 0.0, R, 1));
            BAD(femfct_smooth_cost(ctx, c, Nt, -0.01, R, 1));
            BAD(femfct_smooth_cost(ctx, c, Nt, (double)NAN, R, 1));
            BAD(femfct_smooth_rhs(ctx, nullptr, 1e-3, 1e-6, Nt, 0.01, out, 1));
            BAD(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, 0.01, nullptr, 1));
            BAD(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, 0, 0.01, out, 1));
            BAD(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, 0.01, out, 0));
            BAD(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, 0.0, out, 1));
            BAD(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, (double)INFINITY, out, 1));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, nullptr, u, p, 0.05, 1e-3, 1e-6, 0.01, out, levels, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, nullptr, p, 0.05, 1e-3, 1e-6, 0.01, out, levels, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, nullptr, 0.05, 1e-3, 1e-6, 0.01, out, levels, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.01, nullptr, levels, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.01, out, 1, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.01, out, 0, 1.0, 1.0));
            BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.0, out, levels, 1.0, 1.0));
            for (double bad : {-1e-300, (double)NAN, (double)INFINITY}) {
                BAD(femfct_smooth_rhs(ctx, c, bad, 1e-6, Nt, 0.01, out, 1));
                BAD(femfct_smooth_rhs(ctx, c, 1e-3, bad, Nt, 0.01, out, 1));
                BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, bad, 1e-6, 0.01, out, levels, 1.0, 1.0));
                BAD(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, bad, 0.01, out, levels, 1.0, 1.0));
            }
            OK(femfct_smooth_cost(ctx, c, Nt, 0.01, R, 1));                                                 // still usable
            OK(femfct_smooth_rhs(ctx, c, 1e-3, 1e-6, Nt, 0.01, out, 1));
            OK(femfct_drift_gradient_rhs_smooth(ctx, c, u, p, 0.05, 1e-3, 1e-6, 0.01, out, levels, 1.0, 1.0));
            for (void* q : {(void*)c, (void*)out, (void*)u, (void*)p}) femfct_free(ctx, q);
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[4], R[2];
        BAD(femfct_smooth_cost(ctx, xx, 1, 1.0, R, 1));                                                     // no structured mesh
        BAD(femfct_smooth_rhs(ctx, xx, 1.0, 1.0, 1, 1.0, xx, 1));
        BAD(femfct_drift_gradient_rhs_smooth(ctx, xx, xx, xx, 1.0, 1.0, 1.0, 1.0, xx, 2, 1.0, 1.0));
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_smooth_cost(ctx, xx, 1, 1.0, R, 1));                                                     // a pattern, still no mesh
        BAD(femfct_smooth_rhs(ctx, xx, 1.0, 1.0, 1, 1.0, xx, 1));
        BAD(femfct_drift_gradient_rhs_smooth(ctx, xx, xx, xx, 1.0, 1.0, 1.0, 1.0, xx, 2, 1.0, 1.0));
        const double mvals[2] = {1.0, 1.0};
        OK(femfct_set_mass(ctx, mvals, mvals));
        BAD(femfct_smooth_cost(ctx, xx, 1, 1.0, R, 1));                                                     // a mass, no stiffness
        BAD(femfct_smooth_rhs(ctx, xx, 1.0, 1.0, 1, 1.0, xx, 1));
        femfct_destroy(ctx);
        if (femfct_smooth_cost(nullptr, xx, 1, 1.0, R, 1) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_smooth_rhs(nullptr, xx, 1.0, 1.0, 1, 1.0, xx, 1) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_drift_gradient_rhs_smooth(nullptr, xx, xx, xx, 1.0, 1.0, 1.0, 1.0, xx, 2, 1.0, 1.0) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("smooth_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
