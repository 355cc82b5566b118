// femfct_initial_trials / femfct_initial_trial_stats / femfct_initial_gradient / femfct_omega_gram under AddressSanitizer on
// the fake HIP runtime: the host code that checks the arguments, copies the step and pointer lists into the by-value
// tables, sizes the partials' scratch and the launches, reads 2K doubles back and mirrors the upper triangle, for K = 1
// .. 256, J = 1 .. 17, with and without a background and a mask, member counts that make the scratch grow and then fit, and
// every argument check.  The step, pointer and result lists live on the heap with exactly K, J, 2K and J * J entries: an
// access past them trips the sanitizer.  Kernels do not run.
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
        double *v = dmalloc(ctx, n), *vb = dmalloc(ctx, n), *g = dmalloc(ctx, n);
        uint8_t* mask = (uint8_t*)dmalloc(ctx, ((size_t)n + 7) / 8);
        for (int Nt : {0, 4}) {
            const size_t tl = (size_t)(Nt + 1) * n;
            for (int K : {1, 2, 64, 256, 10, 3}) {     // the scratch grows (64, 256) and then fits (10, 3)
                if (nc == 300 && K > 10) continue;
                double* u = dmalloc(ctx, (size_t)K * tl);
                std::vector<double> steps((size_t)K, 0.5), st(2 * (size_t)K, -1.0);
                OK(femfct_initial_trials(ctx, v, g, steps.data(), K, 0.0, 1.0, u, Nt));
                OK(femfct_initial_trials(ctx, v, g, steps.data(), K, 0.5, 0.5, u, Nt));
                OK(femfct_initial_trial_stats(ctx, u, v, vb, K, Nt, st.data()));
                OK(femfct_initial_trial_stats(ctx, u, v, nullptr, K, Nt, st.data()));
                femfct_free(ctx, u);
            }
            double* p = dmalloc(ctx, tl);
            OK(femfct_initial_gradient(ctx, p, v, vb, 1e-3, g, 0.0, 1.0, mask));
            OK(femfct_initial_gradient(ctx, p, v, nullptr, 0.0, g, 0.0, 0.0, nullptr));
            OK(femfct_initial_gradient(ctx, p, v, vb, 1.0, g, 2.0, 1.0, nullptr));     // no mask: the bounds are not used
            double one[2] = {0.5, 0.25}, st[4];
            BAD(femfct_initial_trials(ctx, nullptr, g, one, 2, 0.0, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, nullptr, one, 2, 0.0, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, nullptr, 2, 0.0, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 2, 0.0, 1.0, nullptr, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 0, 0.0, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 257, 0.0, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 1, 1.0, 0.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 1, NAN, 1.0, p, 0));
            BAD(femfct_initial_trials(ctx, v, g, one, 1, 0.0, 1.0, p, -1));
            BAD(femfct_initial_trial_stats(ctx, nullptr, v, vb, 1, Nt, st));
            BAD(femfct_initial_trial_stats(ctx, p, nullptr, vb, 1, Nt, st));
            BAD(femfct_initial_trial_stats(ctx, p, v, vb, 1, Nt, nullptr));
            BAD(femfct_initial_trial_stats(ctx, p, v, vb, 0, Nt, st));
            BAD(femfct_initial_trial_stats(ctx, p, v, vb, 257, Nt, st));
            BAD(femfct_initial_trial_stats(ctx, p, v, vb, 1, -1, st));
            BAD(femfct_initial_gradient(ctx, nullptr, v, vb, 1.0, g, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, nullptr, vb, 1.0, g, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, v, vb, 1.0, nullptr, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, v, vb, -1.0, g, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, v, vb, NAN, g, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, v, vb, INFINITY, g, 0.0, 1.0, mask));
            BAD(femfct_initial_gradient(ctx, p, v, vb, 1.0, g, 1.0, 0.0, mask));
            OK(femfct_initial_trial_stats(ctx, p, v, vb, 1, Nt, st));                  // still usable
            femfct_free(ctx, p);
        }
        for (int J : {1, 17, 2, 7, 4, 5, 16}) {
            std::vector<const double*> f((size_t)J);
            for (int j = 0; j < J; ++j) f[j] = (j % 3 == 0) ? v : vb;                  // repeated pointers
            std::vector<double> G((size_t)J * J, -1.0);
            OK(femfct_omega_gram(ctx, f.data(), J, nullptr, G.data()));
            OK(femfct_omega_gram(ctx, f.data(), J, mask, G.data()));
        }
        std::vector<const double*> two = {v, vb}, hole = {v, nullptr, vb}, many(18, v);
        std::vector<double> G(18 * 18);
        BAD(femfct_omega_gram(ctx, nullptr, 2, nullptr, G.data()));
        BAD(femfct_omega_gram(ctx, two.data(), 0, nullptr, G.data()));
        BAD(femfct_omega_gram(ctx, two.data(), -3, nullptr, G.data()));
        BAD(femfct_omega_gram(ctx, many.data(), 18, nullptr, G.data()));
        BAD(femfct_omega_gram(ctx, hole.data(), 3, nullptr, G.data()));
        BAD(femfct_omega_gram(ctx, two.data(), 2, nullptr, nullptr));
        OK(femfct_omega_gram(ctx, two.data(), 2, mask, G.data()));                     // still usable
        for (void* q : {(void*)v, (void*)vb, (void*)g, (void*)mask}) femfct_free(ctx, q);
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[2], G[1], s1[1] = {1.0};
        const double* one[1] = {xx};
        BAD(femfct_omega_gram(ctx, one, 1, nullptr, G));                    // no pattern, no mass matrix
        BAD(femfct_initial_trial_stats(ctx, xx, xx, nullptr, 1, 0, xx));
        BAD(femfct_initial_trials(ctx, xx, xx, s1, 1, 0.0, 1.0, xx, 0));    // no mesh: n is not known
        BAD(femfct_initial_gradient(ctx, xx, xx, nullptr, 1.0, xx, 0.0, 1.0, nullptr));
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_omega_gram(ctx, one, 1, nullptr, G));                    // a pattern, still no mass matrix
        BAD(femfct_initial_trial_stats(ctx, xx, xx, nullptr, 1, 0, xx));
        femfct_destroy(ctx);
        if (femfct_omega_gram(nullptr, one, 1, nullptr, G) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_initial_trials(nullptr, xx, xx, s1, 1, 0.0, 1.0, xx, 0) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_initial_trial_stats(nullptr, xx, xx, nullptr, 1, 0, xx) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_initial_gradient(nullptr, xx, xx, nullptr, 1.0, xx, 0.0, 1.0, nullptr) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("initial_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
