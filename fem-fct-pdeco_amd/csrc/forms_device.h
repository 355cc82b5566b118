// Device helpers of the row-gather quadrature forms (kernels_forms.hip, kernels_growth.hip): the node's position, its
// <= 6 triangles, the 7 stencil values of a P1 field, and the chemotaxis flux matrices, which the growth kernels
// (kernels_growth.hip) evaluate in their own launch next to the growth load.  One definition, inlined into every
// kernel that uses it: the same expressions, the same bits.
#pragma once

#include <math.h>

#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "obs_device.h"

namespace {

struct NodeXY { int ix, iy; };

__device__ __forceinline__ NodeXY node_xy(int i, const int32_t* __restrict__ d2v, int N) {
    int v = d2v ? d2v[i] : i;
    return NodeXY{v % N, v / N};
}

template <class F>
__device__ __forceinline__ void for_each_tri(NodeXY p, int nc, F&& f) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const TriInfo T = tri_info(t);
        int cx = p.ix + T.cdx, cy = p.iy + T.cdy;
        if (cx < 0 || cy < 0 || cx >= nc || cy >= nc) continue;
        f(T);
    }
}

// gather the 7 stencil values of a P1 field around row i
__device__ __forceinline__ void gather7(const double* __restrict__ f, const int32_t* __restrict__ cols, int n, int i,
                                        double (&v)[STENCIL_W]) {
    v[0] = f[i];
#pragma unroll
    for (int s = 1; s < STENCIL_W; ++s) v[s] = f[cols[(int64_t)s * n + i]];
}

__device__ __forceinline__ const double* bptr(const VecRef& r, int64_t bstride, int bz) {
    const double* p = vec_ptr(r);
    return p ? p + bz * bstride : nullptr;
}

// What a load form adds to its row's value before it is stored: nothing (the empty tail is inlined away: the forms' own
// kernels keep their machine code), or the level-weighted misfit of a snapshot sweep of the three PDE systems (ObsTerm,
// forms.h): the thread that owns row i adds it as the last term, where the all-time forms add theirs, so theta_n = dt gives
// the all-time bits and theta_n = 0 the final-time bits.  theta is read through the device-side level counter: one captured
// step serves every level, and at theta_n == 0 neither the target nor the state is read (uniform over the grid).
struct NoTail {
    __device__ __forceinline__ double operator()(int, double res) const { return res; }
};

struct ObsTail {
    const MeshArgs& m;
    bool on;                    // the level is observed
    double sc;                  // pre * theta/dt
    const double *a, *b, *w;
    int mass;
    __device__ __forceinline__ double operator()(int i, double res) const {
        if (!on) return res;
        const int n = m.n;
        if (!mass) {
            const double d = a[i] - b[i];
            return res + sc * (w ? w[i] * d : d);
        }
        if (!w) {               // (M (a - b))_i, the expression of form_load's s3 term
            double acc = m.M[i] * (a[i] - b[i]);
#pragma unroll
            for (int s = 1; s < STENCIL_W; ++s) {
                const int64_t idx = (int64_t)s * n + i;
                const int j = m.cols[idx];
                acc += m.M[idx] * (a[j] - b[j]);
            }
            return res + sc * acc;
        }
        double wv[STENCIL_W], dv[STENCIL_W];
        wv[0] = w[i]; dv[0] = a[i] - b[i];
#pragma unroll
        for (int s = 1; s < STENCIL_W; ++s) {
            const int j = m.cols[(int64_t)s * n + i];
            wv[s] = w[j]; dv[s] = a[j] - b[j];
        }
        const double k60 = 0.5 * m.h * m.h / 60.0;
        double r = 0.0;
        for_each_tri(node_xy(i, m.d2v, m.N), m.nc, [&](const TriInfo& T) { r += k60 * p1_triple_term(T, wv, dv); });
        return res + sc * r;
    }
};

__device__ __forceinline__ ObsTail obs_tail(const MeshArgs& m, const ObsTerm& t, int bz) {
    const double* thp = vec_ptr(t.theta);
    const double th = thp ? *thp : 0.0;         // the level's weight: one value for the whole grid
    const bool on = th != 0.0;
    return ObsTail{m, on, t.pre * (th / t.dt), on ? bptr(t.a, t.a_bs, bz) : nullptr, on ? bptr(t.b, t.b_bs, bz) : nullptr,
                   vec_ptr(t.w), t.mass};
}

// ---------------------------------------------------------------------------
// chemotaxis forward flux matrix (helpers.py:1350-1352):
//   A = Dm*Ad - chi * int exp(-eta u_h) (grad v_h . grad phi_i) phi_j      (6-point rule)
// chemotaxis adjoint flux matrix (helpers.py:1499-1503), adjoint != 0:
//   A = Dm*Ad - chi * int (1 - eta u_h) exp(-eta u_h) (grad phi_j . grad v_h) phi_i   (7-point rule)
// ---------------------------------------------------------------------------
template <int ADJ>
__device__ __forceinline__ void form_chtxs_matrix(const MeshArgs& m, VecRef u_ref, int64_t u_bs, VecRef v_ref, int64_t v_bs, double Dm,
                                                  double chi, double eta, double* __restrict__ out_, int bz) {
    const int n = m.n;
    const double* u = bptr(u_ref, u_bs, bz);
    const double* v = bptr(v_ref, v_bs, bz);
    double* out = out_ + (int64_t)bz * STENCIL_W * n;
    const double area = 0.5 * m.h * m.h, ih = 1.0 / m.h;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        NodeXY p = node_xy(i, m.d2v, m.N);
        double uu[STENCIL_W], vv[STENCIL_W];
        gather7(u, m.cols, n, i, uu);
        gather7(v, m.cols, n, i, vv);
        double acc[STENCIL_W] = {0, 0, 0, 0, 0, 0, 0};
        for_each_tri(p, m.nc, [&](const TriInfo& T) {
            double v0 = vv[T.slot[0]], v1 = vv[T.slot[1]], v2 = vv[T.slot[2]];
            double gvx = (v0 * tri_gx(T.type, 0) + v1 * tri_gx(T.type, 1) + v2 * tri_gx(T.type, 2)) * ih;
            double gvy = (v0 * tri_gy(T.type, 0) + v1 * tri_gy(T.type, 1) + v2 * tri_gy(T.type, 2)) * ih;
            double u0 = uu[T.slot[0]], u1 = uu[T.slot[1]], u2 = uu[T.slot[2]];
            if (!ADJ) {
                double gvp = (gvx * tri_gx(T.type, T.pl) + gvy * tri_gy(T.type, T.pl)) * ih;  // grad v . grad phi_P
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    double l0 = quad6_l(q, 0), l1 = quad6_l(q, 1), l2 = quad6_l(q, 2);
                    double e = exp(-eta * (l0 * u0 + l1 * u1 + l2 * u2));
                    double w = quad6_w(q) * area * e * gvp;
                    acc[T.slot[0]] += w * l0;
                    acc[T.slot[1]] += w * l1;
                    acc[T.slot[2]] += w * l2;
                }
            } else {
                double t = 0.0;  // int (1 - eta u) exp(-eta u) phi_P
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    double uq = quad7_l(q, 0) * u0 + quad7_l(q, 1) * u1 + quad7_l(q, 2) * u2;
                    t += quad7_w(q) * area * (1.0 - eta * uq) * exp(-eta * uq) * quad7_l(q, T.pl);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    acc[T.slot[k]] += t * (gvx * tri_gx(T.type, k) + gvy * tri_gy(T.type, k)) * ih;  // grad phi_j . grad v
            }
        });
#pragma unroll
        for (int k = 0; k < STENCIL_W; ++k) {
            int64_t idx = (int64_t)k * n + i;
            out[idx] = Dm * m.Ad[idx] - chi * acc[k];
        }
    }
}

}  // namespace
