// femfct_prox_trials / femfct_l1_norm_Q / femfct_sparse_trial_stats under AddressSanitizer on the fake HIP runtime: the host
// code that checks the arguments, picks the 16-byte or the scalar trial kernel, sizes the partials' scratch and the
// launches and copies the K results back, for K = 1 .. 16, g / src_out present and absent, even and odd counts, batch 1
// and 3, level counts that make the scratch grow and then fit, and every argument check.  The result arrays live on the
// heap with exactly K (or batch) entries: a write past them trips the sanitizer.  Kernels do not run (the results hold
// what the fake copy returns; only their extent is exercised).
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
    for (int nc : {4, 20, 300}) {                      // 300: n > 65536, four waves per block
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, 0));
        const int n = (nc + 1) * (nc + 1);
        for (int Nt : {0, 1, 40, 7, 250, 3}) {         // the scratch grows (40, 250) and then fits (7, 3)
            if (nc == 300 && Nt > 7) continue;
            const int levels = Nt + 1;
            const size_t tl = (size_t)levels * n;
            double *c = dmalloc(ctx, tl), *d = dmalloc(ctx, tl), *g = dmalloc(ctx, tl);
            double *cB = dmalloc(ctx, 16 * tl), *srcB = dmalloc(ctx, 16 * tl);
            for (int K : {1, 16, 2, 10}) {
                std::vector<double> l1((size_t)K, -1.0), dist((size_t)K, -1.0), norm3(3, -1.0), norm1(1, -1.0);
                std::vector<int64_t> nnz((size_t)K, -1);
                OK(femfct_prox_trials(ctx, c, d, g, 1.0, K, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
                OK(femfct_prox_trials(ctx, c, d, nullptr, 1.0, K, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
                OK(femfct_prox_trials(ctx, c, d, g, 1.0, K, 0.0, 0.2, 0.2, (int64_t)tl, cB, nullptr));
                OK(femfct_prox_trials(ctx, c, d, nullptr, 256.0, K, 0.7, -1.0, -0.2, (int64_t)tl, cB, nullptr));
                OK(femfct_prox_trials(ctx, c + 1, d, g, 1.0, K, 1e-3, -0.1, 0.5, (int64_t)tl - 1, cB, srcB));   // not 16-byte aligned
                OK(femfct_prox_trials(ctx, c, d, g, 1.0, K, 1e-3, -0.1, 0.5, 1, cB, srcB));
                OK(femfct_sparse_trial_stats(ctx, cB, c, K, Nt, 0.01, l1.data(), dist.data(), nnz.data()));
                OK(femfct_l1_norm_Q(ctx, cB, Nt, 0.01, norm1.data(), 1));
                OK(femfct_l1_norm_Q(ctx, cB, Nt, 0.01, norm3.data(), 3));
                OK(femfct_l1_norm_Q(ctx, cB, Nt, 0.01, l1.data(), K));
            }
            double l1[16], dist[16];
            int64_t nnz[16];
            BAD(femfct_prox_trials(ctx, nullptr, d, g, 1.0, 2, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, nullptr, g, 1.0, 2, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 2, 1e-3, -0.1, 0.5, (int64_t)tl, nullptr, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 0, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 17, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, -1, 1e-3, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 2, -1e-300, -0.1, 0.5, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 2, 1e-3, 0.5, -0.1, (int64_t)tl, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 2, 1e-3, -0.1, 0.5, 0, cB, srcB));
            BAD(femfct_prox_trials(ctx, c, d, g, 1.0, 2, 1e-3, -0.1, 0.5, -5, cB, srcB));
            BAD(femfct_l1_norm_Q(ctx, nullptr, Nt, 0.01, l1, 1));
            BAD(femfct_l1_norm_Q(ctx, c, Nt, 0.01, nullptr, 1));
            BAD(femfct_l1_norm_Q(ctx, c, -1, 0.01, l1, 1));
            BAD(femfct_l1_norm_Q(ctx, c, Nt, 0.01, l1, 0));
            BAD(femfct_sparse_trial_stats(ctx, nullptr, c, 2, Nt, 0.01, l1, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, nullptr, 2, Nt, 0.01, l1, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 0, Nt, 0.01, l1, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 17, Nt, 0.01, l1, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 2, -1, 0.01, l1, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 2, Nt, 0.01, nullptr, dist, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 2, Nt, 0.01, l1, nullptr, nnz));
            BAD(femfct_sparse_trial_stats(ctx, cB, c, 2, Nt, 0.01, l1, dist, nullptr));
            OK(femfct_sparse_trial_stats(ctx, cB, c, 2, Nt, 0.01, l1, dist, nnz));                        // still usable
            for (void* p : {(void*)c, (void*)d, (void*)g, (void*)cB, (void*)srcB}) femfct_free(ctx, p);
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[2], l1[1], dist[1];
        int64_t nnz[1];
        BAD(femfct_l1_norm_Q(ctx, xx, 0, 1.0, l1, 1));                  // no pattern, no mass matrix
        BAD(femfct_sparse_trial_stats(ctx, xx, xx, 1, 0, 1.0, l1, dist, nnz));
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_l1_norm_Q(ctx, xx, 0, 1.0, l1, 1));                  // a pattern, still no mass matrix
        BAD(femfct_sparse_trial_stats(ctx, xx, xx, 1, 0, 1.0, l1, dist, nnz));
        OK(femfct_prox_trials(ctx, xx, xx, nullptr, 1.0, 1, 0.0, 0.0, 1.0, 2, xx, nullptr));     // needs neither
        femfct_destroy(ctx);
        if (femfct_prox_trials(nullptr, xx, xx, nullptr, 1.0, 1, 0.0, 0.0, 1.0, 2, xx, nullptr) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_l1_norm_Q(nullptr, xx, 0, 1.0, l1, 1) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_sparse_trial_stats(nullptr, xx, xx, 1, 0, 1.0, l1, dist, nnz) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("sparse_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
