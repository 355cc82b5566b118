// The value-by-value prox of the L1-sparse control loops, shared by kernels_sparse.hip (femfct_prox_trials) and
// kernels_budget.hip (femfct_budget_trials), so that both write the same bits for the same threshold.
#pragma once

#include <hip/hip_runtime.h>

// clip(soft_threshold(c + s d, s alpha), lo, hi), evaluated in this order with no contraction (-ffp-contract=off), as
// k_clip_axpy evaluates its clip; alpha = 0 gives k_clip_axpy's value (+0.0 where that has -0.0)
__device__ __forceinline__ double prox_value(double c, double s, double d, double tau, double lo, double hi) {
    const double x = c + s * d;
    const double t = fabs(x) - tau;
    const double v = (t > 0) ? copysign(t, x) : 0.0;
    return fmin(fmax(v, lo), hi);
}
