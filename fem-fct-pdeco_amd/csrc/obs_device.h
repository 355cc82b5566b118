// The windowed mass matrix Mw = assemble(omega_h*u*v*dx) of the snapshot observations, never stored: one triangle's part of
// (Mf(f) x)_P from the exact P1 triple products
//   int_K phi_a phi_b phi_c = |K|/60 * {6: a = b = c, 2: two equal, 1: all different}
// (without the factor |K|/60).  One definition for kernels_obs.hip and the ObsTail of forms_device.h: the same expression, the same bits.
#pragma once

#include "stencil.h"

// fv, xv: the nodal values of f and x on the stencil of P (slot 0 = P); T: a triangle around P
__device__ __forceinline__ double p1_triple_term(const TriInfo& T, const double* fv, const double* xv) {
    const int sq = T.slot[(T.pl + 1) % 3], sr = T.slot[(T.pl + 2) % 3];
    const double fp = fv[0], fq = fv[sq], fr = fv[sr];
    return xv[0] * (6.0 * fp + 2.0 * fq + 2.0 * fr) + xv[sq] * (2.0 * fp + 2.0 * fq + fr) +
           xv[sr] * (2.0 * fp + fq + 2.0 * fr);
}
