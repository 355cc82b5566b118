// femfct_time_restrict / femfct_time_prolong under AddressSanitizer on the fake HIP runtime: the host code that checks
// the interval boundaries, builds the intervals' table (work items, partials, level map) and sizes the scratch and the
// launches, for one interval, one per level, intervals longer than a chunk, tables that grow, shrink and repeat, and
// every argument check.  The boundaries live on the heap with exactly K + 1 entries: a read past them trips the
// sanitizer.  Kernels do not run.
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
    for (int nc : {4, 20}) {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, 0));
        const int n = (nc + 1) * (nc + 1);
        for (int Nt : {1, 6, 250, 31, 700}) {
            const int levels = Nt + 1;
            std::vector<std::vector<int32_t>> sets;
            sets.push_back({0, levels});
            std::vector<int32_t> id(levels + 1);
            for (int l = 0; l <= levels; ++l) id[l] = l;
            sets.push_back(id);
            if (levels > 2) sets.push_back({0, 1, levels});
            if (levels > 4) sets.push_back({0, 3, 4, levels});
            if (levels > 40) sets.push_back({0, 33, 34, levels - 1, levels});
            sets.push_back({0, levels});       // the first table again: uploaded again behind the others
            sets.push_back({0, levels});       // and unchanged: not uploaded
            for (int batch : {1, 3}) {
                double *x = dmalloc(ctx, (size_t)batch * levels * n), *y = dmalloc(ctx, (size_t)batch * levels * n);
                for (const auto& st : sets) {
                    const int K = (int)st.size() - 1;
                    OK(femfct_time_restrict(ctx, x, st.data(), K, Nt, batch, y));
                    OK(femfct_time_prolong(ctx, y, st.data(), K, Nt, batch, x));
                }
                const std::vector<int32_t> one = {0, levels};
                BAD(femfct_time_restrict(ctx, nullptr, one.data(), 1, Nt, batch, y));
                BAD(femfct_time_restrict(ctx, x, nullptr, 1, Nt, batch, y));
                BAD(femfct_time_restrict(ctx, x, one.data(), 1, Nt, batch, nullptr));
                BAD(femfct_time_restrict(ctx, x, one.data(), 0, Nt, batch, y));
                BAD(femfct_time_restrict(ctx, x, one.data(), -1, Nt, batch, y));
                BAD(femfct_time_restrict(ctx, x, one.data(), 1, 0, batch, y));
                BAD(femfct_time_restrict(ctx, x, one.data(), 1, Nt, 0, y));
                BAD(femfct_time_restrict(ctx, x, one.data(), 1, Nt + 1, batch, y));     // wrong end
                BAD(femfct_time_prolong(ctx, nullptr, one.data(), 1, Nt, batch, x));
                BAD(femfct_time_prolong(ctx, y, nullptr, 1, Nt, batch, x));
                BAD(femfct_time_prolong(ctx, y, one.data(), 1, Nt, batch, nullptr));
                BAD(femfct_time_prolong(ctx, y, one.data(), 0, Nt, batch, x));
                BAD(femfct_time_prolong(ctx, y, one.data(), 1, Nt, -2, x));
                const std::vector<int32_t> late = {1, levels}, flat = {0, 1, 1, levels}, back = {0, levels, 1, levels},
                                           many(levels + 3, 0);
                BAD(femfct_time_restrict(ctx, x, late.data(), 1, Nt, batch, y));
                BAD(femfct_time_restrict(ctx, x, flat.data(), 3, Nt, batch, y));
                BAD(femfct_time_prolong(ctx, y, back.data(), 3, Nt, batch, x));
                BAD(femfct_time_prolong(ctx, y, many.data(), levels + 2, Nt, batch, x));   // K > levels
                OK(femfct_time_restrict(ctx, x, one.data(), 1, Nt, batch, y));             // still usable
                femfct_free(ctx, x);
                femfct_free(ctx, y);
            }
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        const int32_t st[2] = {0, 2};
        double xx[1];
        BAD(femfct_time_restrict(ctx, xx, st, 1, 1, 1, xx));      // no pattern registered
        femfct_destroy(ctx);
        if (femfct_time_prolong(nullptr, xx, st, 1, 1, 1, xx) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("time_intervals_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
