// femfct_set_control_zones / femfct_zone_restrict / femfct_zone_prolong under AddressSanitizer on the fake HIP runtime: the
// host code that checks the labels, builds the zone table (offsets, work items, partials, node lists, labels), replaces a
// table by a larger and then a smaller one, sizes the partials' and coefficients' scratch and the launches -- for m = 1
// and m = 256, zones of one chunk and of several, fields = 1 and 3 x 251, with and without the mass rows and the inverse
// Gram matrix, and every argument check, calls without a table included.  The label lists live on the heap with exactly
// n entries: an access past them trips the sanitizer.  Kernels do not run.
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
    for (int nc : {4, 20, 80}) {                       // n = 25, 441, 6561 (a zone of all nodes: seven chunks)
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, 0));
        const int n = (nc + 1) * (nc + 1);
        const int64_t big = 3 * 251;
        double *x = dmalloc(ctx, (size_t)big * n), *s = dmalloc(ctx, (size_t)big * 256), *Ginv = dmalloc(ctx, 256 * 256);
        std::vector<int32_t> lab((size_t)n);
        BAD(femfct_zone_restrict(ctx, x, 1, 0, s));                               // no table yet
        BAD(femfct_zone_prolong(ctx, s, nullptr, 1, x));
        OK(femfct_set_control_zones(ctx, nullptr, 0));                            // clearing nothing
        // m = 1 (one zone of all nodes), a larger table (m = min(n, 256), scattered, some nodes inactive), a smaller one (m = 3)
        for (int m : {1, n < 256 ? n : 256, 3}) {
            for (int i = 0; i < n; ++i) lab[i] = i % m;
            if (m > 1 && n > m) lab[n - 1] = -1;
            OK(femfct_set_control_zones(ctx, lab.data(), m));
            for (int64_t fields : {(int64_t)1, big}) {
                OK(femfct_zone_restrict(ctx, x, fields, 0, s));
                OK(femfct_zone_restrict(ctx, x, fields, 1, s));
                OK(femfct_zone_prolong(ctx, s, Ginv, fields, x));
                OK(femfct_zone_prolong(ctx, s, nullptr, fields, x));
            }
            // a bad table leaves this one in place
            std::vector<int32_t> bad(lab);
            bad[0] = m;
            BAD(femfct_set_control_zones(ctx, bad.data(), m));                    // a label >= m
            bad[0] = -2;
            BAD(femfct_set_control_zones(ctx, bad.data(), m));                    // a label < -1
            BAD(femfct_set_control_zones(ctx, lab.data(), 0));
            BAD(femfct_set_control_zones(ctx, lab.data(), 257));
            BAD(femfct_set_control_zones(ctx, lab.data(), -1));
            if (m < 256 && m < n) BAD(femfct_set_control_zones(ctx, lab.data(), m + 1));     // zone m is empty
            OK(femfct_zone_restrict(ctx, x, 1, 1, s));
            OK(femfct_zone_prolong(ctx, s, Ginv, 1, x));
            BAD(femfct_zone_restrict(ctx, nullptr, 1, 0, s));
            BAD(femfct_zone_restrict(ctx, x, 1, 0, nullptr));
            BAD(femfct_zone_restrict(ctx, x, 0, 0, s));
            BAD(femfct_zone_restrict(ctx, x, -1, 0, s));
            BAD(femfct_zone_restrict(ctx, x, 1, 2, s));
            BAD(femfct_zone_prolong(ctx, nullptr, Ginv, 1, x));
            BAD(femfct_zone_prolong(ctx, s, Ginv, 1, nullptr));
            BAD(femfct_zone_prolong(ctx, s, Ginv, 0, x));
        }
        // one single-node zone with everything else inactive; one node per zone where that fits
        for (int i = 0; i < n; ++i) lab[i] = -1;
        lab[n / 2] = 0;
        OK(femfct_set_control_zones(ctx, lab.data(), 1));
        OK(femfct_zone_restrict(ctx, x, 7, 1, s));
        OK(femfct_zone_prolong(ctx, s, Ginv, 7, x));
        lab[n / 2] = -1;
        BAD(femfct_set_control_zones(ctx, lab.data(), 1));                        // no labelled node at all
        if (n <= 256) {
            for (int i = 0; i < n; ++i) lab[i] = n - 1 - i;
            OK(femfct_set_control_zones(ctx, lab.data(), n));
            OK(femfct_zone_restrict(ctx, x, 3, 1, s));
            OK(femfct_zone_prolong(ctx, s, Ginv, 3, x));
        }
        OK(femfct_set_control_zones(ctx, nullptr, 5));                            // cleared: the calls fail again
        BAD(femfct_zone_restrict(ctx, x, 1, 0, s));
        BAD(femfct_zone_prolong(ctx, s, Ginv, 1, x));
        // a new mesh drops the table
        for (int i = 0; i < n; ++i) lab[i] = 0;
        OK(femfct_set_control_zones(ctx, lab.data(), 1));
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, 3, 0));
        BAD(femfct_zone_restrict(ctx, x, 1, 0, s));
        OK(femfct_set_control_zones(ctx, lab.data(), 1));                         // 16 <= n labels are read
        OK(femfct_zone_restrict(ctx, x, 2, 1, s));
        for (void* q : {(void*)x, (void*)s, (void*)Ginv}) femfct_free(ctx, q);
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);                                                      // with a table registered: freed here
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[2];
        int32_t two[2] = {0, 0};
        BAD(femfct_set_control_zones(ctx, two, 1));                               // no pattern: n is not known
        BAD(femfct_set_control_zones(ctx, nullptr, 0));
        BAD(femfct_zone_restrict(ctx, xx, 1, 0, xx));
        BAD(femfct_zone_prolong(ctx, xx, nullptr, 1, xx));
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        OK(femfct_set_control_zones(ctx, two, 1));
        OK(femfct_zone_restrict(ctx, xx, 1, 0, xx));
        BAD(femfct_zone_restrict(ctx, xx, 1, 1, xx));                             // a pattern, but no mass matrix
        femfct_destroy(ctx);
        if (femfct_set_control_zones(nullptr, two, 1) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_zone_restrict(nullptr, xx, 1, 0, xx) != FEMFCT_ERR_INVALID) fails++;
        if (femfct_zone_prolong(nullptr, xx, nullptr, 1, xx) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("zones_asan_driver: %d unexpected return codes\n", fails);
    return fails != 0;
}
