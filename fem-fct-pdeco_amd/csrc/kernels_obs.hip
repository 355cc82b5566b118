// Tracking a state at chosen time levels (snapshot observations), the load and the cost of
//   J = 1/2 sum_n w_n (u_n - uhat_n)^T Mw (u_n - uhat_n),    Mw = assemble(omega_h*u*v*dx)  (M without a window omega).
// The discrete adjoint of the backward-Euler step for J loads the step to level n with (theta_n/dt) Mw (uhat_n - u_n) and
// ends in p_Nt = tau omega (uhat_Nt - u_Nt) (nodal, as the reference's terminal condition); the two modes of the reference
// are its corners, (tau, theta) = (1, 0) (advection_solidbody_FCT_PDECO_finaltime.py:200-221) and (0, dt)
// (..._alltime.py:232-259, whose load FCT_alg_ref multiplies by dt).
//
//   k_obs_load      out = (theta[level]/dt) Mw (a - b) [- Mg(g) x]: the load launch of an adjoint step, theta read through
//                   the device-side level counter.  theta[level] == 0: a and b are not read (uniform over the grid), so the
//                   target needs data at observed levels only.  Without a window the M (a - b) part is k_mass_diff's
//                   expression (kernels_asm.hip), the reaction part k_react_load's (kernels_react.hip): theta = dt and
//                   theta = 0 give those kernels' bits.
//   k_obs_terminal  p_Nt = tau omega (uhat_Nt - u_Nt)
//   k_obs_cost_part / k_obs_cost_finish   the cost per batch member: per-block partials on a grid that depends on n only,
//                   then one finishing block -- a fixed order, the same bits at every batch size.
// Mw is never stored: the thread owning row P visits the <= 6 triangles around P with the exact P1 triple products
//   int_K phi_a phi_b phi_c = |K|/60 * {6: a = b = c, 2: two equal, 1: all different}.
// One thread per row, fields gathered through the ELL column table (either DoF ordering), no atomics.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "solidbody_op.h"
#include "obs_device.h"
#include "obs_load_device.h"

#include <algorithm>

namespace {

__global__ void k_obs_load(MeshArgs m, ObsLoadSpec sp, double* __restrict__ out_) {
    const int bz = blockIdx.y, n = m.n;
    const double th = *vec_ptr(sp.theta);       // the level's weight: one value for the whole grid
    const bool observed = th != 0.0;
    const double scale = th / sp.dt;
    const double* a = observed ? obs_member(sp.a, sp.a_bs, bz) : nullptr;
    const double* b = observed ? obs_member(sp.b, sp.b_bs, bz) : nullptr;
    const double* w = vec_ptr(sp.w);            // window, may be absent: Mw = M
    const double* g = obs_member(sp.g, 0, bz);      // reaction coefficient, may be absent: no Mg(g) x term
    const double* x = obs_member(sp.x, sp.x_bs, bz);
    double* out = out_ + (int64_t)bz * n;
    const double k60 = 0.5 * m.h * m.h / 60.0;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        OBS_LOAD_ROW(acc)       // reads m, n, i, k60, observed, scale, a, b, w, g, x by name (obs_load_device.h)
        out[i] = acc;
    }
}

__global__ void k_obs_terminal(int n, double tau, const double* __restrict__ w, const double* __restrict__ uhat,
                               int64_t uhat_bs, const double* __restrict__ u, int64_t u_bs, double* __restrict__ p,
                               int64_t p_bs) {
    const int bz = blockIdx.y;
    const double *hb = uhat + bz * uhat_bs, *ub = u + bz * u_bs;
    double* pb = p + bz * p_bs;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double d = hb[i] - ub[i];
        pb[i] = tau * (w ? w[i] * d : d);
    }
}

// part[bz * gridDim.x + blockIdx.x] = sum over the block's rows and the observed levels of w_n d_i (Mw d)_i, d = u_n - uhat_n
__global__ void __launch_bounds__(256) k_obs_cost_part(MeshArgs m, const double* __restrict__ u_, const double* __restrict__ uhat_,
                                                       int64_t tstride, const double* __restrict__ cw,
                                                       const double* __restrict__ w, int levels, double* __restrict__ part) {
    __shared__ double smem[32];
    const int bz = blockIdx.y, n = m.n;
    const double k60 = 0.5 * m.h * m.h / 60.0;
    RowRange rr = block_rows(n);
    double sum = 0.0;
    for (int lvl = 0; lvl < levels; ++lvl) {
        const double wt = cw[lvl];
        if (wt == 0.0) continue;                // uniform: an unobserved level is not read
        const double* u = u_ + bz * tstride + (int64_t)lvl * n;
        const double* uh = uhat_ + bz * tstride + (int64_t)lvl * n;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            double dv[STENCIL_W], wv[STENCIL_W];
            dv[0] = u[i] - uh[i];
            wv[0] = w ? w[i] : 1.0;
            double r = m.M[i] * dv[0];
#pragma unroll
            for (int s = 1; s < STENCIL_W; ++s) {
                const int64_t idx = (int64_t)s * n + i;
                const int j = m.cols[idx];
                dv[s] = u[j] - uh[j];
                wv[s] = w ? w[j] : 1.0;
                r += m.M[idx] * dv[s];
            }
            if (w) r = obs_weighted_mass_row(node_xy(i, m.d2v, m.N), m.nc, k60, wv, dv);
            sum += wt * (dv[0] * r);
        }
    }
    sum = block_reduce(sum, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) part[(int64_t)bz * gridDim.x + blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256) k_obs_cost_finish(const double* __restrict__ part, int count, int batch,
                                                         double* __restrict__ out) {
    __shared__ double smem[32];
    for (int b = 0; b < batch; ++b) {
        const double v = reduce_partials(part + (int64_t)b * count, count, OpSum(), 0.0, smem);
        if (threadIdx.x == 0) out[b] = 0.5 * v;
    }
}

}  // namespace

int femfct_enqueue_obs_load(femfct_ctx* ctx, const ObsLoadSpec& sp, double* out, int32_t batch) {
    LaunchGeom g = femfct_geom(ctx, batch);
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_obs_load, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), sp, out);
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

int femfct_enqueue_obs_terminal(femfct_ctx* ctx, double tau, const double* window, const double* uhat, int64_t uhat_bs,
                                const double* u, int64_t u_bs, double* p, int64_t p_bs, int32_t batch) {
    const int bs = 256;
    int64_t g = ((int64_t)ctx->n + bs - 1) / bs;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_obs_terminal, dim3((unsigned)g, (unsigned)batch), dim3(bs), 0, ctx->stream, ctx->n, tau, window, uhat,
                       uhat_bs, u, u_bs, p, p_bs);
    return FEMFCT_OK;
}

extern "C" {

int femfct_obs_load(femfct_ctx* ctx, const double* a_dev, const double* b_dev, const double* theta_dev, int32_t level,
                    double dt, const double* window_dev, double* out_dev, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, theta_dev, "theta is null");
    ARG_TRY(ctx, a_dev && b_dev && out_dev && level >= 0 && dt > 0 && batch >= 1 && batch <= 65535, "bad argument");
    ObsLoadSpec sp;
    sp.a = make_ref(a_dev); sp.a_bs = ctx->n;
    sp.b = make_ref(b_dev); sp.b_bs = ctx->n;
    sp.theta = make_ref(theta_dev + level);
    sp.w = make_ref(window_dev);
    sp.dt = dt;
    femfct_enqueue_obs_load(ctx, sp, out_dev, batch);
    HIP_TRY(ctx, hipGetLastError());
    return FEMFCT_OK;
}

int femfct_obs_cost(femfct_ctx* ctx, const double* u_traj, const double* uhat_traj, const double* cost_w_dev,
                    const double* window_dev, int32_t num_steps, int32_t batch, double* out_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, cost_w_dev, "cost_w is null");
    ARG_TRY(ctx, u_traj && uhat_traj && out_host && num_steps >= 1 && batch >= 1 && batch <= 65535, "bad argument");
    // the grid depends on n alone: a member's partials, and so its cost, are the same bits at every batch size
    const int blocks = (int)std::min<int64_t>(1024, ((int64_t)ctx->n + 255) / 256);
    double* d_ws = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_ws, sizeof(double) * ((size_t)blocks + 1) * batch));
    double* d_out = d_ws + (size_t)blocks * batch;
    hipLaunchKernelGGL(k_obs_cost_part, dim3(blocks, batch), dim3(256), 0, ctx->stream, femfct_mesh_args(ctx), u_traj, uhat_traj,
                       (int64_t)(num_steps + 1) * ctx->n, cost_w_dev, window_dev, num_steps + 1, d_ws);
    hipLaunchKernelGGL(k_obs_cost_finish, dim3(1), dim3(256), 0, ctx->stream, d_ws, blocks, batch, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_out, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d_ws);
    HIP_TRY(ctx, e);
    return FEMFCT_OK;
}

}  // extern "C"
