// femfct_budget_trials under AddressSanitizer on the fake HIP runtime: the host code that checks the arguments, sizes the
// scratch of the writing pass and of the search rounds, launches, copies the K results back and runs the search loop, for
// K = 1 and 16 (and 2, 10), g / src_out / d present and NULL, level counts that make the scratch grow and then fit,
// every rejected argument and a NULL context.  The result arrays live on the heap with exactly K entries: a write past
// them trips the sanitizer.  Kernels do not run, so a call here reads back whatever the fake device memory holds (zeros:
// every trial within the budget); the verdict on a round's read-back, femfct_budget_narrow, is therefore also driven
// directly, with arbitrary values -- NaN, infinities, negative sums, nonsensical counts, random bits -- to show that the
// search of a trial ends within the round cap, with a threshold inside its bracket, whatever comes back.
#include "femfct_internal.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define OK(x) do { int rc_ = (x); if (rc_ != FEMFCT_OK) { printf("line %d: rc %d (%s)\n", __LINE__, rc_, femfct_last_error(ctx)); fails++; } } while (0)
#define BAD(x) do { int rc_ = (x); if (rc_ != FEMFCT_ERR_INVALID) { printf("line %d: rc %d, expected FEMFCT_ERR_INVALID\n", __LINE__, rc_); fails++; } } while (0)

static double* dmalloc(femfct_ctx* ctx, size_t count) {
    void* p = nullptr;
    if (femfct_malloc(ctx, &p, count * sizeof(double)) != FEMFCT_OK) abort();
    femfct_memset0(ctx, p, count * sizeof(double));
    return (double*)p;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_bits() {       // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static double arbitrary(int kind) {
    const double special[] = {0.0, -0.0, NAN, INFINITY, -INFINITY, 1e308, -1e308, 5e-324, 1.0, -1.0, 0.5, 1e-3};
    if (kind % 3 == 0) return special[next_bits() % 12];
    if (kind % 3 == 1) return (double)(next_bits() >> 11) * (1.0 / 9007199254740992.0);     // [0, 1)
    const uint64_t b = next_bits();                                                         // any bit pattern
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// the loop of femfct_budget_trials for one trial, fed with arbitrary read-backs
static int search_terminates() {
    int fails = 0;
    const double brackets[][2] = {{0.0, 1.0}, {1e-3, 40.0}, {0.25, 0.25}, {1.0, 0.5}, {0.0, 5e-324}, {1.0, nextafter(1.0, 2.0)},
                                  {0.0, 1e308}, {3.0, INFINITY}};
    for (int trial = 0; trial < 20000; ++trial) {
        const double a0 = brackets[trial % 8][0], b0 = brackets[trial % 8][1];
        double a = a0, b = b0, th = NAN;
        bool done = false;
        int round = 0;
        for (round = 1; round <= BUDGET_MAX_ROUNDS && !done; ++round) {
            std::vector<double> v(BUDGET_VALS);             // exactly the values the verdict may read
            for (int j = 0; j < BUDGET_VALS; ++j) v[j] = arbitrary(trial + j + round);
            if (trial % 5 == 0) v[BUDGET_SUMS] = 7.0;       // a count that never lets the closed form in: narrowing only
            done = femfct_budget_narrow(&a, &b, v.data(), 0.1, &th);
            if (!done && !(a >= a0 && b <= b0 && b > a)) { printf("bracket [%g, %g] left [%g, %g]\n", a, b, a0, b0); fails++; break; }
        }
        if (!done) th = b;                                  // the round cap
        if (b0 > a0 && !(th >= a0 && th <= b0)) { printf("threshold %g outside [%g, %g]\n", th, a0, b0); fails++; }
        if (!(b0 > a0) && !(done && round == 2)) { printf("empty bracket not ended at once\n"); fails++; }
    }
    // a monotone phi that never becomes affine in the count's eyes: the bracket shrinks 16-fold a round
    double a = 0.0, b = 1.0, th = NAN;
    int rounds = 0;
    for (bool done = false; !done && rounds < BUDGET_MAX_ROUNDS; ++rounds) {
        double v[BUDGET_VALS];
        for (int j = 0; j < BUDGET_POINTS; ++j) v[j] = 1.0 - (a + (b - a) * ((j + 1) * 0.0625));      // phi(theta) = 1 - theta
        v[BUDGET_POINTS] = v[BUDGET_POINTS + 1] = v[BUDGET_POINTS + 2] = 0.0;
        v[BUDGET_SUMS] = 1.0;
        done = femfct_budget_narrow(&a, &b, v, 0.3, &th);
    }
    if (!(a <= 0.7 + 1e-15 && 0.7 - 1e-15 <= b && b - a < 1e-14)) { printf("narrowing lost the root: [%.17g, %.17g]\n", a, b); fails++; }
    // the closed form on an affine bracket: phi = 0.2 + 1.5 - 2 theta = 0.3 at theta = 0.7
    a = 0.0; b = 1.0;
    double v[BUDGET_VALS] = {0};
    v[BUDGET_POINTS] = 0.2; v[BUDGET_POINTS + 1] = 1.5; v[BUDGET_POINTS + 2] = 2.0; v[BUDGET_SUMS] = 0.0;
    if (!femfct_budget_narrow(&a, &b, v, 0.3, &th) || fabs(th - 0.7) > 1e-15) { printf("closed form: %g\n", th); fails++; }
    return fails;
}

int main() {
    int fails = search_terminates();
    for (int nc : {4, 20, 300}) {                      // 300: n > 65536, four waves per block
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) { printf("create failed\n"); return 1; }
        OK(femfct_set_mesh_square(ctx, -1.0, 1.0, nc, 0));
        const int n = (nc + 1) * (nc + 1);
        for (int Nt : {0, 1, 40, 7, 250, 3}) {         // the scratch grows (40, 250) and then fits (7, 3)
            if (nc == 300 && Nt > 7) continue;
            const size_t tl = (size_t)(Nt + 1) * n;
            double *c = dmalloc(ctx, tl), *d = dmalloc(ctx, tl), *g = dmalloc(ctx, tl);
            double *cB = dmalloc(ctx, 16 * tl), *srcB = dmalloc(ctx, 16 * tl);
            for (int K : {1, 16, 2, 10}) {
                std::vector<double> lam((size_t)K, -1.0), l1((size_t)K, -1.0);
                std::vector<int32_t> rounds((size_t)K, -1);
                OK(femfct_budget_trials(ctx, c, d, g, 1.0, K, 1e-3, 0.1, -0.1, 0.5, Nt, 0.01, cB, srcB, lam.data(), l1.data(), rounds.data()));
                OK(femfct_budget_trials(ctx, c, d, nullptr, 1.0, K, 1e-3, 0.1, -0.1, 0.5, Nt, 0.01, cB, srcB, lam.data(), l1.data(), rounds.data()));
                OK(femfct_budget_trials(ctx, c, d, g, 256.0, K, 0.0, 1e300, 0.0, 0.0, Nt, 0.01, cB, nullptr, lam.data(), l1.data(), rounds.data()));
                OK(femfct_budget_trials(ctx, c, d, nullptr, 1.0, K, 0.7, 5e-324, -1e9, 1e9, Nt, 0.01, cB, nullptr, lam.data(), l1.data(), rounds.data()));
                for (int t = 0; t < K; ++t)
                    if (lam[t] != 0.0 || rounds[t] != 0) { printf("line %d: a trial of zeros searched\n", __LINE__); fails++; }
                if (K == 1)
                    OK(femfct_budget_trials(ctx, c, nullptr, g, 1.0, 1, 0.0, 0.1, -0.1, 0.5, Nt, 0.01, cB, srcB, lam.data(), l1.data(), rounds.data()));
                else
                    BAD(femfct_budget_trials(ctx, c, nullptr, g, 1.0, K, 0.0, 0.1, -0.1, 0.5, Nt, 0.01, cB, srcB, lam.data(), l1.data(), rounds.data()));
            }
            double lam[16], l1[16];
            int32_t rounds[16];
#define CALL(c_, cB_, K_, alpha_, B_, lo_, hi_, Nt_, lam_, l1_, r_) \
    femfct_budget_trials(ctx, c_, d, g, 1.0, K_, alpha_, B_, lo_, hi_, Nt_, 0.01, cB_, srcB, lam_, l1_, r_)
            BAD(CALL(nullptr, cB, 2, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, nullptr, 2, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, -0.1, 0.5, Nt, nullptr, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, -0.1, 0.5, Nt, lam, nullptr, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, nullptr));
            BAD(CALL(c, cB, 0, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 17, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, -1, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, -1e-300, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, NAN, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.0, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, -0.1, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, NAN, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, INFINITY, -0.1, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, 0.1, 0.5, Nt, lam, l1, rounds));          // boxes without 0
            BAD(CALL(c, cB, 2, 1e-3, 0.1, -0.5, -0.1, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, 0.5, -0.1, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, NAN, 0.5, Nt, lam, l1, rounds));
            BAD(CALL(c, cB, 2, 1e-3, 0.1, -0.1, 0.5, -1, lam, l1, rounds));
            OK(CALL(c, cB, 2, 1e-3, 0.1, -0.1, 0.5, Nt, lam, l1, rounds));          // still usable
            for (void* p : {(void*)c, (void*)d, (void*)g, (void*)cB, (void*)srcB}) femfct_free(ctx, p);
        }
        OK(femfct_synchronize(ctx));
        femfct_destroy(ctx);
    }
    {
        femfct_ctx* ctx = nullptr;
        if (femfct_create(&ctx, 0) != FEMFCT_OK) return 1;
        double xx[2], lam[1], l1[1];
        int32_t rounds[1];
        BAD(femfct_budget_trials(ctx, xx, xx, nullptr, 1.0, 1, 0.0, 0.1, 0.0, 1.0, 0, 1.0, xx, nullptr, lam, l1, rounds));   // no pattern, no mass
        const int32_t indptr[3] = {0, 1, 2}, indices[2] = {0, 1};
        OK(femfct_set_pattern_csr(ctx, 2, indptr, indices));
        BAD(femfct_budget_trials(ctx, xx, xx, nullptr, 1.0, 1, 0.0, 0.1, 0.0, 1.0, 0, 1.0, xx, nullptr, lam, l1, rounds));   // a pattern, no mass
        femfct_destroy(ctx);
        if (femfct_budget_trials(nullptr, xx, xx, nullptr, 1.0, 1, 0.0, 0.1, 0.0, 1.0, 0, 1.0, xx, nullptr, lam, l1, rounds) != FEMFCT_ERR_INVALID) fails++;
    }
    printf("budget_asan_driver: %d unexpected results\n", fails);
    return fails != 0;
}
