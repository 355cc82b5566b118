// Device primitives of the ensemble drift control (solvers.ensemble_solidbody; an extension, no reference call): one
// control c serves S scenarios, each with its own state u_s, FCT adjoint p_s, target and weight pi_s >= 0,
//   J(c) = sum_s pi_s T_s(u_s(c)) + beta/2 ||c||^2_Q,      T_s the tracking term of femfct_obs_cost.
//   femfct_ensemble_drift_gradient_rhs   rhs = -(beta M c + sum_s pi_s assemble(p_s (b.grad u_s) v dx)), every level, one
//                                        launch: the direction then takes one mass solve per level whatever S is
//   femfct_ensemble_costs                T_s of every scenario, J, ||c||^2_Q and ||c - cref||^2_Q with one read-back
// The weights enter here and not in the adjoint loads: the limiter makes p_s a nonlinear function of its load.
//
// No atomics anywhere.  The sums run in the fixed trees of the kernels they restate (k_drift_gradient_rhs in
// kernels_asm.hip, k_obs_cost_part / k_obs_cost_finish in kernels_obs.hip, k_quadform / k_reduce_levels in
// kernels_pgd.hip), so the results are those entry points' bit for bit; a scenario of weight 0 is never read by the rhs.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "solidbody_op.h"
#include "obs_device.h"
#include "obs_load_device.h"

#include <algorithm>
#include <cmath>

namespace {

// The scenarios of non-zero weight, in index order, passed by value in the kernel arguments (as MemberTable in
// kernels_pgd.hip): no device buffer to own, fill or synchronise on.  2.5 KiB.
struct EnsembleTable {
    double w[FEMFCT_MAX_MEMBERS];
    uint16_t idx[FEMFCT_MAX_MEMBERS];
};

// Scenarios whose gathers are in flight together.  2: 122 VGPRs, four waves per SIMD, no scratch; 4: 202 VGPRs, two waves,
// the same 112 gathers in flight per SIMD and twice the code.
#ifndef ENS_U
#define ENS_U 2
#endif

// the 7 values of u_s and p_s around row i (slot 0 = the row itself)
struct EnsRing { double u[STENCIL_W], p[STENCIL_W]; };

__device__ __forceinline__ EnsRing ens_gather(const double* __restrict__ u, const double* __restrict__ pv, int i,
                                              const int (&col)[STENCIL_W]) {
    EnsRing r;
    r.u[0] = u[i]; r.p[0] = pv[i];
#pragma unroll
    for (int s = 1; s < STENCIL_W; ++s) {
        r.u[s] = u[col[s]];
        r.p[s] = pv[col[s]];
    }
    return r;
}

// row P of assemble(p_h (b.grad u_h) v dx): k_drift_gradient_rhs's expression (triangle order, m12, divisions)
__device__ __forceinline__ double ens_row_gradient(NodeXY p, int nc, double h, double m12, double bx, double by,
                                                   const EnsRing& r) {
    double g = 0.0;
    for_each_tri(p, nc, [&](const TriInfo& T, int, int) {
        double u0 = r.u[T.slot[0]], u1 = r.u[T.slot[1]], u2 = r.u[T.slot[2]];
        double gux = (u0 * tri_gx(T.type, 0) + u1 * tri_gx(T.type, 1) + u2 * tri_gx(T.type, 2)) / h;
        double guy = (u0 * tri_gy(T.type, 0) + u1 * tri_gy(T.type, 1) + u2 * tri_gy(T.type, 2)) / h;
        double psum = r.p[T.slot[0]] + r.p[T.slot[1]] + r.p[T.slot[2]];
        g += (bx * gux + by * guy) * m12 * (r.p[0] + psum);   // (M_K p_K)_P, P is slot 0
    });
    return g;
}

// out_l = -(beta M c_l + ((pi_a0 g_a0 + pi_a1 g_a1) + ...)) over the `active` scenarios of the table, blockIdx.y = time
// level.  A row loads its columns and forms (M c)_i once; the scenarios follow ENS_U at a time, their 14 gathers each
// issued before the first is used.  tl = levels * n, the distance between two scenarios.
__global__ void __launch_bounds__(256)
k_ensemble_drift_gradient_rhs(int n, int N, int nc, double h, const int32_t* __restrict__ d2v,
                              const int32_t* __restrict__ cols, const double* __restrict__ M,
                              const double* __restrict__ c_, const double* __restrict__ u_,
                              const double* __restrict__ p_, int64_t tl, EnsembleTable tab, int active, double beta,
                              double bx, double by, double* __restrict__ out_) {
    const int64_t voff = (int64_t)blockIdx.y * n;
    const double* c = c_ + voff;
    const double *u = u_ + voff, *pv = p_ + voff;
    double* out = out_ + voff;
    RowRange rr = block_rows(n);
    const double m12 = 0.5 * h * h / 12.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        NodeXY p = node_xy(i, d2v, N);
        int col[STENCIL_W];
        col[0] = i;
        double mc = M[i] * c[i];
#pragma unroll
        for (int s = 1; s < STENCIL_W; ++s) {
            int64_t idx = (int64_t)s * n + i;
            col[s] = cols[idx];
            mc += M[idx] * c[col[s]];
        }
        // the first scenario starts the sum, the others are added in index order
        int a = 0;
        double acc;
        {
            const int64_t o = (int64_t)tab.idx[0] * tl;
            acc = tab.w[0] * ens_row_gradient(p, nc, h, m12, bx, by, ens_gather(u + o, pv + o, i, col));
            a = 1;
        }
        for (; a + ENS_U <= active; a += ENS_U) {
            EnsRing r[ENS_U];
#pragma unroll
            for (int k = 0; k < ENS_U; ++k) {
                const int64_t o = (int64_t)tab.idx[a + k] * tl;
                r[k] = ens_gather(u + o, pv + o, i, col);
            }
#pragma unroll
            for (int k = 0; k < ENS_U; ++k) acc = acc + tab.w[a + k] * ens_row_gradient(p, nc, h, m12, bx, by, r[k]);
        }
        for (; a < active; ++a) {
            const int64_t o = (int64_t)tab.idx[a] * tl;
            acc = acc + tab.w[a] * ens_row_gradient(p, nc, h, m12, bx, by, ens_gather(u + o, pv + o, i, col));
        }
        out[i] = -(beta * mc + acc);
    }
}

// k_obs_cost_part's partial for every scenario: part[s * gridDim.x + block] = sum over the block's rows and the observed
// levels of w_n d_i (Mw d)_i, d = u_{s,n} - uhat_{s,n}.  The grid's x extent depends on n alone and a scenario's levels are
// summed inside its item, as femfct_obs_cost sums them: the same bits at every S.  Scenarios are strided over gridDim.y.
__global__ void __launch_bounds__(256) k_ensemble_track_part(MeshArgs m, const double* __restrict__ u_,
                                                             const double* __restrict__ uhat_, int64_t tstride,
                                                             const double* __restrict__ cw, const double* __restrict__ w,
                                                             int levels, int S, double* __restrict__ part) {
    __shared__ double smem[32];
    const int n = m.n;
    const double k60 = 0.5 * m.h * m.h / 60.0;
    RowRange rr = block_rows(n);
    for (int bz = blockIdx.y; bz < S; bz += gridDim.y) {
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
}

// The control's two quadratic forms in one pass, c read once: for every level (strided over gridDim.y) and block
// k_quadform's partials of phi = c - 0 (as femfct_l2_norm_sq_Q(c, NULL) forms it) and, with cref, of phi = c - cref.
// Rows, expressions and order are k_quadform's (block_rows partition, diagonal then slots 1..W-1, block_reduce from 0.0).
__global__ void k_ensemble_control_part(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ M,
                                        const double* __restrict__ c, const double* __restrict__ cref, int levels,
                                        double* __restrict__ part_c, double* __restrict__ part_d) {
    __shared__ double smem[2 * 32];
    RowRange rr = block_rows(n);
    for (int lvl = blockIdx.y; lvl < levels; lvl += gridDim.y) {
        const double* cl = c + (int64_t)lvl * n;
        const double* rl = cref ? cref + (int64_t)lvl * n : nullptr;
        double sc = 0.0, sd = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double ci = cl[i];
            const double pc = ci - 0.0, pd = rl ? ci - rl[i] : 0.0;
            double ac = M[i] * pc, ad = M[i] * pd;
            for (int k = 1; k < W; ++k) {
                const int64_t idx = (int64_t)k * n + i;
                const int j = cols[idx];
                const double mk = M[idx], cj = cl[j];
                ac += mk * (cj - 0.0);
                if (rl) ad += mk * (cj - rl[j]);
            }
            sc += pc * ac;
            sd += pd * ad;
        }
        sc = block_reduce(sc, OpSum(), 0.0, smem);
        if (rl) sd = block_reduce(sd, OpSum(), 0.0, smem + 32);
        if (threadIdx.x == 0) {
            const int64_t pl = (int64_t)lvl * gridDim.x + blockIdx.x;
            part_c[pl] = sc;
            if (rl) part_d[pl] = sd;
        }
    }
}

// blocks 0..S-1: out[s] = T_s as k_obs_cost_finish folds it; block S: out[S] = ||c||^2_Q and block S + 1:
// out[S + 1] = ||c - cref||^2_Q as k_reduce_levels folds them (trapezoid, scale dt, from 0.0)
__global__ void __launch_bounds__(256) k_ensemble_finish(const double* __restrict__ part_t, int Gt, int S,
                                                         const double* __restrict__ part_c,
                                                         const double* __restrict__ part_d, int levels, int G, double dt,
                                                         double* __restrict__ out) {
    __shared__ double smem[32];
    const int b = blockIdx.x;
    if (b < S) {
        const double v = reduce_partials(part_t + (int64_t)b * Gt, Gt, OpSum(), 0.0, smem);
        if (threadIdx.x == 0) out[b] = 0.5 * v;
        return;
    }
    const double* p = b == S ? part_c : part_d;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < (int64_t)levels * G; k += blockDim.x) {
        int l = (int)(k / G);
        double w = (l == 0 || l == levels - 1) ? 0.5 : 1.0;
        s += w * p[k];
    }
    s = block_reduce(s, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) out[b] = 0.0 + dt * s;
}

// Checks the S weights and lists the scenarios of non-zero weight in index order; returns their number (0: invalid)
int ensemble_table(const double* weights, int32_t S, EnsembleTable* tab) {
    memset(tab, 0, sizeof(*tab));
    int active = 0;
    for (int s = 0; s < S; ++s) {
        const double w = weights[s];
        if (!(w >= 0.0) || !std::isfinite(w)) return 0;
        if (w == 0.0) continue;
        tab->w[active] = w;
        tab->idx[active] = (uint16_t)s;
        ++active;
    }
    return active;
}

}  // namespace

extern "C" {

int femfct_ensemble_drift_gradient_rhs(femfct_ctx* ctx, const double* c_dev, const double* u_traj, const double* p_traj,
                                       const double* weights_host, int32_t S, double beta, double bx, double by,
                                       double* out_dev, int32_t levels) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->structured, "structured mesh not set");
    ARG_TRY(ctx, c_dev && u_traj && p_traj && weights_host && out_dev, "null argument");
    ARG_TRY(ctx, levels >= 1 && levels <= 65535, "levels must be in 1..65535");
    ARG_TRY(ctx, S >= 1 && S <= FEMFCT_MAX_MEMBERS, "S (scenarios) must be in 1..256");
    EnsembleTable tab;
    const int active = ensemble_table(weights_host, S, &tab);
    ARG_TRY(ctx, active >= 1, "weights must be finite and >= 0 with a positive sum");
    LaunchGeom g = femfct_geom(ctx, levels);
    hipLaunchKernelGGL(k_ensemble_drift_gradient_rhs, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->N, ctx->n_cells,
                       ctx->h, ctx->d_d2v, ctx->d_cols, ctx->d_M, c_dev, u_traj, p_traj, (int64_t)levels * ctx->n, tab,
                       active, beta, bx, by, out_dev);
    return FEMFCT_OK;
}

int femfct_ensemble_costs(femfct_ctx* ctx, const double* u_traj, const double* uhat_traj, const double* cost_w_dev,
                          const double* window_dev, const double* c_dev, const double* cref_dev,
                          const double* weights_host, int32_t S, double beta, int32_t num_steps, double dt,
                          double* T_host, double* J_host, double* dist_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->structured && ctx->have_mass, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, u_traj && uhat_traj && cost_w_dev && c_dev && weights_host && T_host && J_host, "null argument");
    ARG_TRY(ctx, (cref_dev == nullptr) == (dist_host == nullptr), "cref and dist_host must be given together");
    ARG_TRY(ctx, num_steps >= 1, "num_steps must be >= 1");
    ARG_TRY(ctx, S >= 1 && S <= FEMFCT_MAX_MEMBERS, "S (scenarios) must be in 1..256");
    EnsembleTable tab;
    const int active = ensemble_table(weights_host, S, &tab);
    ARG_TRY(ctx, active >= 1, "weights must be finite and >= 0 with a positive sum");
    const int levels = num_steps + 1;
    // femfct_obs_cost's grid for the tracking partials, femfct_l2_norm_sq_Q's for the control's: each depends on n alone
    const int Gt = (int)std::min<int64_t>(1024, ((int64_t)ctx->n + 255) / 256);
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t pt = (size_t)Gt * S, pc = (size_t)levels * G;
    int rc = femfct_ensure_scratch(ctx, pt + 2 * pc + (size_t)S + 2);
    if (rc != FEMFCT_OK) return rc;
    double *part_t = ctx->d_scratch, *part_c = part_t + pt, *part_d = part_c + pc, *res = part_d + pc;
    hipLaunchKernelGGL(k_ensemble_track_part, dim3(Gt, (unsigned)S), dim3(256), 0, ctx->stream, femfct_mesh_args(ctx),
                       u_traj, uhat_traj, (int64_t)levels * ctx->n, cost_w_dev, window_dev, levels, (int)S, part_t);
    g.grid.y = (unsigned)levels;      // (num_steps + 1 <= 65535 levels fit; more are strided)
    if (levels > 65535) g.grid.y = 65535;
    hipLaunchKernelGGL(k_ensemble_control_part, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M,
                       c_dev, cref_dev, levels, part_c, part_d);
    hipLaunchKernelGGL(k_ensemble_finish, dim3((unsigned)(S + (cref_dev ? 2 : 1))), dim3(256), 0, ctx->stream, part_t, Gt,
                       (int)S, part_c, part_d, levels, G, dt, res);
    HIP_TRY(ctx, hipGetLastError());
    double host[FEMFCT_MAX_MEMBERS + 2];
    const size_t count = (size_t)S + (cref_dev ? 2 : 1);
    HIP_TRY(ctx, hipMemcpyAsync(host, res, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < S; ++s) T_host[s] = host[s];
    double track = tab.w[0] * host[tab.idx[0]];
    for (int a = 1; a < active; ++a) track = track + tab.w[a] * host[tab.idx[a]];
    J_host[0] = track + (0.5 * beta) * host[S];
    if (dist_host) dist_host[0] = host[S + 1];
    return FEMFCT_OK;
}

}  // extern "C"
