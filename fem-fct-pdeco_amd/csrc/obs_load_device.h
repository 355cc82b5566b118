// The row of the snapshot load, scale * Mw(w) (a - b) - Mg(g) x: one definition for k_obs_load (kernels_obs.hip) and
// k_bound_load (kernels_bounds.hip), the same expression, the same bits.
#pragma once

#include "stencil.h"
#include "forms.h"
#include "solidbody_op.h"
#include "obs_device.h"

// (Mf(f) x)_P with the nodal values of f and x on the stencil of P (slot 0 = P)
__device__ __forceinline__ double obs_weighted_mass_row(const NodeXY& P, int nc, double k60, const double* fv, const double* xv) {
    double r = 0.0;
    for_each_tri(P, nc, [&](const TriInfo& T, int, int) {
        const double t = p1_triple_term(T, fv, xv);
        r += k60 * t;
    });
    return r;
}

// member bz of a batched vector reference (null stays null)
__device__ __forceinline__ const double* obs_member(const VecRef& r, int64_t bstride, int bz) {
    const double* p = vec_ptr(r);
    return p ? p + bz * bstride : nullptr;
}

// Row i of scale * Mw(w) (a - b) - Mg(g) x into the double `acc`, as statements: the launches that share them (k_obs_load,
// k_bound_load) compile the same token stream, so k_obs_load keeps its machine code.  In scope where it is used: MeshArgs m,
// int n = m.n, int i, double k60, bool observed (false: a and b are not read), double scale, const double *a, *b, *w (absent:
// Mw = M), *g (absent: no reaction term), *x.  The macro takes these eleven names from the caller's scope: a kernel that
// uses it keeps them, and says so where it does.
#define OBS_LOAD_ROW(acc)                                                                              \
    double acc = 0.0;                                                                                  \
    if (observed && !w) {                                                                              \
        acc = m.M[i] * (a[i] - b[i]);                                                                  \
        _Pragma("unroll") for (int s = 1; s < STENCIL_W; ++s) {                                        \
            const int64_t idx = (int64_t)s * n + i;                                                    \
            const int j = m.cols[idx];                                                                 \
            acc += m.M[idx] * (a[j] - b[j]);                                                           \
        }                                                                                              \
        acc = scale * acc;                                                                             \
    } else if (observed) {                                                                             \
        double wv[STENCIL_W], dv[STENCIL_W];                                                           \
        wv[0] = w[i]; dv[0] = a[i] - b[i];                                                             \
        _Pragma("unroll") for (int s = 1; s < STENCIL_W; ++s) {                                        \
            const int j = m.cols[(int64_t)s * n + i];                                                  \
            wv[s] = w[j]; dv[s] = a[j] - b[j];                                                         \
        }                                                                                              \
        acc = scale * obs_weighted_mass_row(node_xy(i, m.d2v, m.N), m.nc, k60, wv, dv);                \
    }                                                                                                  \
    if (g) {                                                                                           \
        double gv[STENCIL_W], xv[STENCIL_W];                                                           \
        gv[0] = g[i]; xv[0] = x[i];                                                                    \
        _Pragma("unroll") for (int s = 1; s < STENCIL_W; ++s) {                                        \
            const int j = m.cols[(int64_t)s * n + i];                                                  \
            gv[s] = g[j]; xv[s] = x[j];                                                                \
        }                                                                                              \
        acc = acc - obs_weighted_mass_row(node_xy(i, m.d2v, m.N), m.nc, k60, gv, xv);                  \
    }
