// Load vector of the explicit (IMEX) reaction term of the linear source-control problem:
//   out_i = (M (a - b))_i - sum_j (int g_h phi_i phi_j) x_j
// (advection_FCT_PDECO_finaltime_exact.py:273-277 state / sensitivity, :317-321 adjoint: u_rhs = assemble(src*v*dx),
// Mg = assemble_sparse(g_fun*u*v*dx), u_rhs -= Mg @ u_n).  Matrix-free: the thread owning row P visits the <= 6 triangles
// around P (stencil.h) with the exact P1 triple products
//   int_K phi_a phi_b phi_c = |K|/60 * {6: a = b = c, 2: two equal, 1: all different},
// so Mg is never stored.  Field values are gathered through the ELL column table: either DoF ordering works.  One thread
// per row, a fixed summation order (the same bits batched and alone), no atomics.  The M (a - b) part is k_mass_diff's
// expression (kernels_asm.hip), so with g = 0 the result has the bits of that kernel.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "solidbody_op.h"

namespace {

__device__ __forceinline__ const double* member(const VecRef& r, int64_t bstride, int bz) {
    const double* p = vec_ptr(r);
    return p ? p + bz * bstride : nullptr;
}

__global__ void k_react_load(MeshArgs m, ReactLoadSpec sp, double* __restrict__ out_) {
    const int bz = blockIdx.y, n = m.n;
    const double* a = member(sp.a, sp.a_bs, bz);     // may be absent: no M (a - b) term
    const double* b = member(sp.b, sp.b_bs, bz);     // may be absent: M a
    const double* g = member(sp.g, sp.g_bs, bz);
    const double* x = member(sp.x, sp.x_bs, bz);
    double* out = out_ + (int64_t)bz * n;
    const double k60 = 0.5 * m.h * m.h / 60.0;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double gv[STENCIL_W], xv[STENCIL_W];
        gv[0] = g[i]; xv[0] = x[i];
        double acc = a ? m.M[i] * (a[i] - (b ? b[i] : 0.0)) : 0.0;
#pragma unroll
        for (int s = 1; s < STENCIL_W; ++s) {
            const int64_t idx = (int64_t)s * n + i;
            const int j = m.cols[idx];
            gv[s] = g[j]; xv[s] = x[j];
            if (a) acc += m.M[idx] * (a[j] - (b ? b[j] : 0.0));
        }
        double react = 0.0;
        for_each_tri(node_xy(i, m.d2v, m.N), m.nc, [&](const TriInfo& T, int, int) {
            // P = local node pl (ELL slot 0); q, r: the triangle's other two nodes
            const int sq = T.slot[(T.pl + 1) % 3], sr = T.slot[(T.pl + 2) % 3];
            const double gp = gv[0], gq = gv[sq], gr = gv[sr];
            const double t = xv[0] * (6.0 * gp + 2.0 * gq + 2.0 * gr) + xv[sq] * (2.0 * gp + 2.0 * gq + gr) +
                             xv[sr] * (2.0 * gp + gq + 2.0 * gr);
            react += k60 * t;
        });
        out[i] = acc - react;
    }
}

}  // namespace

int femfct_enqueue_react_load(femfct_ctx* ctx, const ReactLoadSpec& sp, double* out, int32_t batch) {
    LaunchGeom g = femfct_geom(ctx, batch);
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_react_load, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), sp, out);
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

extern "C" {

int femfct_react_load(femfct_ctx* ctx, const double* src_dev, const double* g_dev, const double* x_dev, double* out_dev,
                      int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, g_dev && x_dev && out_dev && batch >= 1 && batch <= 65535, "bad argument");
    ReactLoadSpec sp;
    sp.a = make_ref(src_dev); sp.a_bs = ctx->n;
    sp.g = make_ref(g_dev);   sp.g_bs = 0;           // one coefficient for the whole batch
    sp.x = make_ref(x_dev);   sp.x_bs = ctx->n;
    femfct_enqueue_react_load(ctx, sp, out_dev, batch);
    HIP_TRY(ctx, hipGetLastError());
    return FEMFCT_OK;
}

int femfct_assemble_weighted_mass(femfct_ctx* ctx, const double* f_dev, double* out_ell) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, f_dev && out_ell, "null argument");
    // assemble(f_h*u*v*dx) = the weighted-mass form int f1_h f2_h phi_i phi_j with f2 = 1 (cubic: the 6-point rule is exact)
    std::vector<double> one((size_t)ctx->n, 1.0);
    double* d_one = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_one, sizeof(double) * one.size()));
    hipError_t e = hipMemcpyAsync(d_one, one.data(), sizeof(double) * one.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        WMassSpec ws;
        ws.beta = 1.0;
        ws.f1 = make_ref(f_dev);
        ws.f2 = make_ref(d_one);
        femfct_enqueue_weighted_mass(ctx, ws, out_ell, 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d_one);
    HIP_TRY(ctx, e);
    return FEMFCT_OK;
}

}  // extern "C"
