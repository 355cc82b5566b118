// Load vectors of the explicit (IMEX) cell-growth term of the chemotaxis system,
//   du/dt + div(-Dm grad u + chi u exp(-eta u) grad v) = r(u),   r(u) = u (r0 + r1 u + r2 u^2)
// (chemotaxis_mimura_FCT_PGD_alltime.py header: m (4 - m); mimura_data_helpers.py:65-70: m^2 (1 - m), "using IMEX so that
// the reaction term is on the RHS"):
//   out_i = s1 * int q1_h q2_h phi_i + s2 * (da_i - db_i) + int (g0 + g1 a_h + g2 a_h^2) a_h^e b_h phi_i
//   forward  a = u_n, e = 1, b = 1,       g = (r0, r1, r2):      int r(u_n) phi_i, the right-hand side of the FCT step
//   adjoint  a = u_n, e = 0, b = p_{n+1}, g = (r0, 2 r1, 3 r2):  int r'(u_n) p_{n+1} phi_i, next to the terms the step's
//            load has without growth, c_n q_{n+1} / rescaling and the raw nodal misfit uhat_n - u_n (helpers.py:1505-1507)
// Row-gather like the forms of kernels_forms.hip: the thread owning row P visits the <= 6 triangles around P, field
// values come through the ELL column table (either DoF ordering), the integrands have degree <= 4 and the 6-point rule is
// exact for them.  One thread per row, a fixed summation order (the same bits batched and alone), no atomics.
// A step keeps its launch count: k_chtxs_matrix_growth evaluates the step's chemotaxis flux matrix (blockIdx.z = 0, the
// function k_chtxs_matrix runs: forms_device.h) and the growth load (blockIdx.z = 1) in one launch.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "forms_device.h"

namespace {

template <class Tail = NoTail>
__device__ __forceinline__ void form_growth_load(const MeshArgs& m, const GrowthLoadSpec& sp, double* __restrict__ out_, int bz,
                                                 Tail tail = Tail()) {
    const int n = m.n;
    const double* a = bptr(sp.a, sp.a_bs, bz);
    const double* b = bptr(sp.b, sp.b_bs, bz);       // may be absent: 1
    const double* q1 = bptr(sp.q1, sp.q1_bs, bz);    // may be absent: no product term
    const double* q2 = bptr(sp.q2, sp.q2_bs, bz);
    const double* da = bptr(sp.da, sp.da_bs, bz);    // may be absent: no nodal difference
    const double* db = bptr(sp.db, sp.db_bs, bz);
    double* out = out_ + (int64_t)bz * n;
    const double area = 0.5 * m.h * m.h;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        NodeXY p = node_xy(i, m.d2v, m.N);
        double av[STENCIL_W], bv[STENCIL_W], c1[STENCIL_W], c2[STENCIL_W];
        gather7(a, m.cols, n, i, av);
        if (b) gather7(b, m.cols, n, i, bv);
        if (q1) { gather7(q1, m.cols, n, i, c1); gather7(q2, m.cols, n, i, c2); }
        double ld = 0.0, gr = 0.0;
        for_each_tri(p, m.nc, [&](const TriInfo& T) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double l0 = quad6_l(q, 0), l1 = quad6_l(q, 1), l2 = quad6_l(q, 2);
                const double w = quad6_w(q) * area * quad6_l(q, T.pl);
                const double aq = l0 * av[T.slot[0]] + l1 * av[T.slot[1]] + l2 * av[T.slot[2]];
                double f = sp.g0 + aq * (sp.g1 + sp.g2 * aq);
                if (sp.e) f *= aq;
                if (b) f *= l0 * bv[T.slot[0]] + l1 * bv[T.slot[1]] + l2 * bv[T.slot[2]];
                gr += w * f;
                if (q1)
                    ld += w * ((l0 * c1[T.slot[0]] + l1 * c1[T.slot[1]] + l2 * c1[T.slot[2]]) *
                               (l0 * c2[T.slot[0]] + l1 * c2[T.slot[1]] + l2 * c2[T.slot[2]]));
            }
        });
        double res = gr;
        if (q1) res += sp.s1 * ld;
        if (da) res += sp.s2 * (da[i] - (db ? db[i] : 0.0));
        out[i] = tail(i, res);
    }
}

__global__ void k_growth_load(MeshArgs m, GrowthLoadSpec sp, double* __restrict__ out_) { form_growth_load(m, sp, out_, blockIdx.y); }

template <int ADJ>
__global__ void k_chtxs_matrix_growth(MeshArgs m, ChtxsMatSpec c, double* __restrict__ mat_out, GrowthLoadSpec sp,
                                      double* __restrict__ load_out) {
    if (blockIdx.z == 0) form_chtxs_matrix<ADJ>(m, c.u, c.u_bs, c.v, c.v_bs, c.p0, c.p1, c.p2, mat_out, blockIdx.y);
    else form_growth_load(m, sp, load_out, blockIdx.y);
}

// the adjoint launch with the snapshot misfit of the cell density in the load (ObsTail, forms_device.h)
// z0 = 0, gridDim.z = 2: the adjoint flux matrix and the load; z0 = 1, gridDim.z = 1: the load alone
// (blocks of 64 or 256 threads, femfct_geom: with the bound the growth load and the windowed misfit fit the register file;
// without it the compiler assumes 1024 threads, 128 VGPRs, and spills 15 of them)
__global__ void __launch_bounds__(256) k_chtxs_matrix_growth_obs(MeshArgs m, ChtxsMatSpec c, double* __restrict__ mat_out, GrowthLoadSpec sp, ObsTerm t,
                                          double* __restrict__ load_out, int z0) {
    if (blockIdx.z + z0 == 0) form_chtxs_matrix<1>(m, c.u, c.u_bs, c.v, c.v_bs, c.p0, c.p1, c.p2, mat_out, blockIdx.y);
    else form_growth_load(m, sp, load_out, blockIdx.y, obs_tail(m, t, blockIdx.y));
}

}  // namespace

int femfct_enqueue_growth_load(femfct_ctx* ctx, const GrowthLoadSpec& sp, double* out, int32_t batch) {
    LaunchGeom g = femfct_geom(ctx, batch);
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_growth_load, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), sp, out);
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

int femfct_enqueue_chtxs_matrix_growth(femfct_ctx* ctx, int adjoint, const ChtxsMatSpec& c, double* mat_out,
                                       const GrowthLoadSpec& sp, double* load_out, int32_t batch) {
    if (!ctx->form_groups) {      // FEMFCT_FORM_GROUPS=0: each form in its own launch -- the same functions, the same bits
        int r = femfct_enqueue_chtxs_matrix(ctx, adjoint, c.u, c.u_bs, c.v, c.v_bs, c.p0, c.p1, c.p2, mat_out, batch);
        if (r != FEMFCT_OK) return r;
        return femfct_enqueue_growth_load(ctx, sp, load_out, batch);
    }
    LaunchGeom g = femfct_geom(ctx, batch);
    g.grid.z = 2;
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    if (adjoint)
        hipLaunchKernelGGL(k_chtxs_matrix_growth<1>, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), c, mat_out, sp, load_out);
    else
        hipLaunchKernelGGL(k_chtxs_matrix_growth<0>, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), c, mat_out, sp, load_out);
    femfct_prof_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return femfct_fail(ctx, FEMFCT_ERR_HIP, "growth form launch failed: %s", hipGetErrorString(e));
    return FEMFCT_OK;
}

int femfct_enqueue_chtxs_matrix_growth_obs(femfct_ctx* ctx, const ChtxsMatSpec& c, double* mat_out, const GrowthLoadSpec& sp,
                                           const ObsTerm& t, double* load_out, int32_t batch) {
    LaunchGeom g = femfct_geom(ctx, batch);
    int z0 = 0;
    if (!ctx->form_groups) {      // FEMFCT_FORM_GROUPS=0: the matrix in its own launch, then the load alone -- the same bits
        int r = femfct_enqueue_chtxs_matrix(ctx, 1, c.u, c.u_bs, c.v, c.v_bs, c.p0, c.p1, c.p2, mat_out, batch);
        if (r != FEMFCT_OK) return r;
        z0 = 1;
    } else {
        g.grid.z = 2;
    }
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_chtxs_matrix_growth_obs, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), c, mat_out, sp, t,
                       load_out, z0);
    femfct_prof_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return femfct_fail(ctx, FEMFCT_ERR_HIP, "growth form launch failed: %s", hipGetErrorString(e));
    return FEMFCT_OK;
}
