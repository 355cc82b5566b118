// What the three families of multi-sweep kernels share (kernels_rowstrip.hip, kernels_tile32.hip, kernels_patch64.hip):
// the workgroup size, the by-value omega table of a Chebyshev launch and the run-time -> compile-time dispatch of
// their launchers and the launch loop of a Chebyshev solve.  Kernels live in exactly one of the three files, never here.
#pragma once

#include <algorithm>
#include <type_traits>

#define STRIP_T 1024

namespace {   // (per translation unit, as the kernels that take it by value: their mangled names carry the namespace)

struct CheOmegas { double w[24]; };   // omegas of one launch (up to TILE_HMAX iterations; all 19 of ChebSI on a single patch)

// f(std::integral_constant<int, v>()) for the run-time v in LO .. HI; any other value takes HI.  The launchers pick a
// kernel instantiation with it: every value of LO .. HI instantiates the generic lambda f once.
template <int LO, int HI, class F>
void with_constant(int v, F&& f) {
    if constexpr (LO < HI) {
        if (v != LO) return with_constant<LO + 1, HI>(v, f);
    }
    f(std::integral_constant<int, LO>());
}

// Chebyshev iterations k_first..k_last (1-based, inclusive) in ceil(count / per_launch) launches:
// launch(k0, k1, om, mid, old, omid, oold) enqueues iterations k0..k1-1 with their omegas in om (no omegas: zeros).
// in_mid = y_{k_first-1} (null = 0), in_old = y_{k_first-2} (null = 0); result y_{k_last} -> y_out.
// pairs (bufA0,bufA1)/(bufB0,bufB1) are alternated as intermediate (mid, old) storage.
template <class F>
void for_cheb_launches(int k_first, int k_last, int per_launch, const double* omegas, const double* mid, const double* old,
                       double* y_out, double* bufA0, double* bufA1, double* bufB0, double* bufB1, F&& launch) {
    int which = 0;
    for (int k0 = k_first; k0 <= k_last; k0 += per_launch) {
        const int k1 = std::min(k_last + 1, k0 + per_launch);
        CheOmegas om;     // (more than 24 iterations per launch: the kernel reads its omegas from device memory)
        for (int k = k0; k < k1 && k - k0 < 24; ++k) om.w[k - k0] = omegas ? omegas[k - 1] : 0.0;
        const bool last = (k1 == k_last + 1);
        double* omid = last ? y_out : (which ? bufB0 : bufA0);
        double* oold = last ? nullptr : (which ? bufB1 : bufA1);
        launch(k0, k1, om, mid, old, omid, oold);
        mid = omid;
        old = oold;
        which ^= 1;
    }
}

}  // namespace
