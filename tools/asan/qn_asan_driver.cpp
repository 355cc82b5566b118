// femfct_free_set / femfct_q_gram / femfct_q_combine under AddressSanitizer on the fake HIP runtime: the host code that
// checks the arguments, copies the pointer and coefficient lists into the by-value tables, sizes the partials' scratch
// and the launches and mirrors the upper triangle, for J = 1 .. 17, with and without a mask, a repeated pointer, level
// counts that make the scratch grow and then fit, and every argument check.  The pointer and coefficient lists live on
// the heap with exactly J entries: a read past them trips the sanitizer.  Kernels do not run (G holds what the fake
// copy returns; only its J * J extent is exercised).
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
            double *a = dmalloc(ctx, tl), *b = dmalloc(ctx, tl), *out = dmalloc(ctx, tl);
            uint8_t* mask = (uint8_t*)dmalloc(ctx, (tl + 7) / 8);
            OK(femfct_free_set(ctx, a, b, 0.0, 1.0, (int64_t)tl, mask));
            OK(femfct_free_set(ctx, a, b, 0.0, 1.0, 0, mask));
            for (int J : {1, 17, 2, 11, 4, 5, 16}) {
                std::vector<const double*> f((size_t)J);
                for (int j = 0; j < J; ++j) f[j] = (j % 3 == 0) ? a : b;       // repeated pointers
                std::vector<double> coef((size_t)J, 0.5), G((size_t)J * J, -1.0);
                OK(femfct_q_gram(ctx, f.data(), J, nullptr, Nt, 0.01, G.data()));
                OK(femfct_q_gram(ctx, f.data(), J, mask, Nt, 0.01, G.data()));
                OK(femfct_q_combine(ctx, f.data(), coef.data(), J, nullptr, nullptr, 0.0, (int64_t)tl, out));
                OK(femfct_q_combine(ctx, f.data(), coef.data(), J, mask, a, -1.0, (int64_t)tl, out));
            }
            std::vector<const double*> two = {a, b}, hole = {a, nullptr, b}, many(18, a);
            std::vector<double> c2 = {1.0, -1.0}, c18(18, 1.0), G(18 * 18);
            BAD(femfct_free_set(ctx, nullptr, b, 0.0, 1.0, (int64_t)tl, mask));
            BAD(femfct_free_set(ctx, a, nullptr, 0.0, 1.0, (int64_t)tl, mask));
            BAD(femfct_free_set(ctx, a, b, 0.0, 1.0, (int64_t)tl, nullptr));
            BAD(femfct_free_set(ctx, a, b, 0.0, 1.0, -1, mask));
            BAD(femfct_q_gram(ctx, nullptr, 2, nullptr, Nt, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, two.data(), 0, nullptr, Nt, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, two.data(), -3, nullptr, Nt, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, many.data(), 18, nullptr, Nt, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, hole.data(), 3, nullptr, Nt, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, two.data(), 2, nullptr, -1, 0.01, G.data()));
            BAD(femfct_q_gram(ctx, two.data(), 2, nullptr, Nt, 0.01, nullptr));
            BAD(femfct_q_combine(ctx, nullptr, c2.data(), 2, nullptr, nullptr, 0.0, (int64_t)tl, out));
            BAD(femfct_q_combine(ctx, two.data(), nullptr, 2, nullptr, nullptr, 0.0, (int64_t)tl, out));
            BAD(femfct_q_combine(ctx, two.data(), c2.data(), 0, nullptr, nullptr, 0.0, (int64_t)tl, out));
            BAD(femfct_q_combine(ctx, many.data(), c18.data(), 18, nullptr, nullptr, 0.0, (int64_t)tl, out));
            BAD(femfct_q_combine(ctx, hole.data(), c18.data(), 3, nullptr, nullptr, 0.0, (int64_t)tl, out));
            BAD(femfct_q_combine(ctx, two.data(), c2.data(), 2, mask, nullptr, -1.0, (int64_t)tl, out));   // mask, no fallback
            BAD(femfct_q_combine(ctx, two.data(), c2.data(), 2, nullptr, nullptr, 0.0, -1, out));
            BAD(femfct_q_combine(ctx, two.data(), c2.data(), 2, nullptr, nullptr, 0.0, (int64_t)tl, nullptr));
            OK(femfct_q_gram(ctx, two.data(), 2, mask, Nt, 0.01, G.data()));                              // still usable
            for (void* p : {(void*)a, (void*)b, (void*)out, (void*)mask}) femfct_free(ctx, p);
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[1], G[1];
        const double* one[1] = {xx};
        BAD(femfct_q_gram(ctx, one, 1, nullptr, 0, 1.0, G));            // no pattern, no mass matrix
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_q_gram(ctx, one, 1, nullptr, 0, 1.0, G));            // a pattern, still no mass matrix
        femfct_destroy(ctx);
        if (femfct_q_gram(nullptr, one, 1, nullptr, 0, 1.0, G) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_free_set(nullptr, xx, xx, 0.0, 1.0, 1, (uint8_t*)xx) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_q_combine(nullptr, one, xx, 1, nullptr, nullptr, 0.0, 1, xx) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("qn_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
