// Smooth controls (solvers.Smoothness; an extension, no reference call): the H1 seminorm of a control trajectory
// c = (c_0 .. c_Nt) in space and time, with the trapezoid's level weights w_l (1/2 at the two end levels, 1 otherwise),
//   R(c) = beta_x/2 R_x + beta_t/2 R_t
//   R_x  = dt sum_{l=0..Nt} w_l c_l^T Ad c_l                            Ad = assemble(grad u . grad v dx), ctx->d_Ad
//   R_t  = (1/dt) sum_{l<Nt} (c_{l+1} - c_l)^T M (c_{l+1} - c_l)        M the mass of femfct_l2_norm_sq_Q
// and its gradient g in that call's inner product, dR(c)[v] = dt sum_l w_l g_l^T M v_l:
//   M g_l = beta_x Ad c_l + beta_t M tau_l,    tau_l = (2 c_l - c_{l-1} - c_{l+1}) / dt^2  (0 < l < Nt),
//   tau_0 = 2 (c_0 - c_1) / dt^2,  tau_Nt = 2 (c_Nt - c_{Nt-1}) / dt^2
// (the end weights 1/2 double the one-sided difference), the per-level form of the existing beta M c_l.
//
//   femfct_smooth_cost               (R_x, R_t) per batch member: one partials launch over (member, level, row block) that
//                                    forms both quadratic forms in one pass over c, then the two level folds
//   femfct_smooth_rhs                out_l = -(beta_x Ad c_l + beta_t M tau_l), every level and member, one launch
//   femfct_drift_gradient_rhs_smooth k_drift_gradient_rhs's row and smooth_row in one launch
// One thread per row of the block_rows partition; no atomics; the sums run in the fixed trees of k_quadform and
// k_reduce_levels (kernels_pgd.hip), so every call returns the same bits.  A zero beta_t reads no neighbouring level, a
// zero beta_x no Ad.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "solidbody_op.h"

#include <cmath>
#include <vector>

namespace {

// the levels tau_l reads besides l: l - 1 and l + 1, at an end level the one neighbour twice, so that
// (2 c_l - c_lo) - c_hi is 2 (c_l - c_nb) there
__device__ __forceinline__ int level_below(int l) { return l > 0 ? l - 1 : 1; }
__device__ __forceinline__ int level_above(int l, int levels) { return l < levels - 1 ? l + 1 : levels - 2; }

// (beta_x Ad c_l + beta_t M tau_l)_i.  cl, clo, chi: the levels l, level_below(l), level_above(l) of one trajectory;
// col: the row's columns (col[0] = i); inv_dt2 = 1 / dt^2.  The coefficients are uniform over the launch.
__device__ __forceinline__ double smooth_row(int n, int i, const int (&col)[STENCIL_W], const double* __restrict__ Ad,
                                             const double* __restrict__ M, const double* __restrict__ cl,
                                             const double* __restrict__ clo, const double* __restrict__ chi, double bx,
                                             double bt, double inv_dt2) {
    double ax = 0.0, mt = 0.0;
    if (bx != 0.0) {
        ax = Ad[i] * cl[i];
#pragma unroll
        for (int s = 1; s < STENCIL_W; ++s) ax += Ad[(int64_t)s * n + i] * cl[col[s]];
    }
    if (bt != 0.0) {
        mt = M[i] * ((2.0 * cl[i] - clo[i]) - chi[i]);
#pragma unroll
        for (int s = 1; s < STENCIL_W; ++s) {
            const int j = col[s];
            mt += M[(int64_t)s * n + i] * ((2.0 * cl[j] - clo[j]) - chi[j]);
        }
    }
    if (bx != 0.0 && bt != 0.0) return bx * ax + bt * (mt * inv_dt2);
    if (bx != 0.0) return bx * ax;
    if (bt != 0.0) return bt * (mt * inv_dt2);
    return 0.0;
}

// out = -smooth_row for the items (member, level), strided over gridDim.y; a member's levels are contiguous
__global__ void __launch_bounds__(256) k_smooth_rhs(int n, const int32_t* __restrict__ cols, const double* __restrict__ Ad,
                                                    const double* __restrict__ M, const double* __restrict__ c_, int levels,
                                                    int64_t items, double bx, double bt, double inv_dt2,
                                                    double* __restrict__ out_) {
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int l = (int)(q % levels);
        const double* base = c_ + (q - l) * n;              // level 0 of the item's member
        const double *cl = base + (int64_t)l * n, *clo = base + (int64_t)level_below(l) * n,
                     *chi = base + (int64_t)level_above(l, levels) * n;
        double* out = out_ + q * n;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            int col[STENCIL_W];
            col[0] = i;
#pragma unroll
            for (int s = 1; s < STENCIL_W; ++s) col[s] = cols[(int64_t)s * n + i];
            out[i] = -smooth_row(n, i, col, Ad, M, cl, clo, chi, bx, bt, inv_dt2);
        }
    }
}

// k_drift_gradient_rhs's row (kernels_asm.hip: the same expression and order for beta M c and the drift gradient g) and
// smooth_row in one pass: out = -(beta mc + g) - sm, the sum femfct_axpby(1, drift rhs, 1, smooth rhs) forms (a negation
// is exact, one addition).  smooth == 0 (both coefficients zero): -(beta mc + g), that kernel's bits.
__global__ void __launch_bounds__(256)
k_drift_gradient_rhs_smooth(int n, int N, int nc, double h, const int32_t* __restrict__ d2v,
                            const int32_t* __restrict__ cols, const double* __restrict__ M, const double* __restrict__ Ad,
                            const double* __restrict__ c_, const double* __restrict__ u_, const double* __restrict__ p_,
                            int levels, double beta, double bx_s, double bt_s, double inv_dt2, int smooth, double bx,
                            double by, double* __restrict__ out_) {
    RowRange rr = block_rows(n);
    const double m12 = 0.5 * h * h / 12.0;
    for (int l = blockIdx.y; l < levels; l += gridDim.y) {
        const int64_t voff = (int64_t)l * n;
        const double *c = c_ + voff, *u = u_ + voff, *pv = p_ + voff;
        const double *clo = c_ + (int64_t)level_below(l) * n, *chi = c_ + (int64_t)level_above(l, levels) * n;
        double* out = out_ + voff;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            NodeXY p = node_xy(i, d2v, N);
            int col[STENCIL_W];
            double uv[STENCIL_W], pp[STENCIL_W];
            col[0] = i;
            uv[0] = u[i]; pp[0] = pv[i];
            double mc = M[i] * c[i];
#pragma unroll
            for (int s = 1; s < STENCIL_W; ++s) {
                int64_t idx = (int64_t)s * n + i;
                int j = cols[idx];
                col[s] = j;
                uv[s] = u[j];
                pp[s] = pv[j];
                mc += M[idx] * c[j];
            }
            double g = 0.0;
            for_each_tri(p, nc, [&](const TriInfo& T, int, int) {
                double u0 = uv[T.slot[0]], u1 = uv[T.slot[1]], u2 = uv[T.slot[2]];
                double gux = (u0 * tri_gx(T.type, 0) + u1 * tri_gx(T.type, 1) + u2 * tri_gx(T.type, 2)) / h;
                double guy = (u0 * tri_gy(T.type, 0) + u1 * tri_gy(T.type, 1) + u2 * tri_gy(T.type, 2)) / h;
                double psum = pp[T.slot[0]] + pp[T.slot[1]] + pp[T.slot[2]];
                g += (bx * gux + by * guy) * m12 * (pp[0] + psum);   // (M_K p_K)_P, P is slot 0
            });
            const double dr = -(beta * mc + g);
            out[i] = smooth ? dr - smooth_row(n, i, col, Ad, M, c, clo, chi, bx_s, bt_s, inv_dt2) : dr;
        }
    }
}

// For the items (member, level), strided over gridDim.y, and every row block the partials of both quadratic forms,
//   part_x[q G + blk] = sum_i c_l,i (Ad c_l)_i          part_t[q G + blk] = sum_i d_i (M d)_i,  d = c_{l+1} - c_l
// (the last level: 0, c_{l+1} is not read) in one pass over c_l's rows: rows, slot order and the block tree are k_quadform's.
__global__ void __launch_bounds__(256) k_smooth_cost_part(int n, const int32_t* __restrict__ cols,
                                                          const double* __restrict__ Ad, const double* __restrict__ M,
                                                          const double* __restrict__ c_, int levels, int64_t items,
                                                          double* __restrict__ part_x, double* __restrict__ part_t) {
    __shared__ double smem[2 * 32];
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int l = (int)(q % levels);
        const bool last = l == levels - 1;                  // uniform over the block
        const double* cl = c_ + q * n;
        const double* cn = cl + n;
        double sx = 0.0, st = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double ci = cl[i], di = last ? 0.0 : cn[i] - ci;
            double ax = Ad[i] * ci, mt = M[i] * di;
#pragma unroll
            for (int s = 1; s < STENCIL_W; ++s) {
                const int64_t idx = (int64_t)s * n + i;
                const int j = cols[idx];
                const double cj = cl[j];
                ax += Ad[idx] * cj;
                if (!last) mt += M[idx] * (cn[j] - cj);
            }
            sx += ci * ax;
            st += di * mt;
        }
        sx = block_reduce(sx, OpSum(), 0.0, smem);
        st = block_reduce(st, OpSum(), 0.0, smem + 32);
        if (threadIdx.x == 0) {
            part_x[q * gridDim.x + blockIdx.x] = sx;
            part_t[q * gridDim.x + blockIdx.x] = st;
        }
    }
}

bool coefficient_ok(double b) { return b >= 0.0 && std::isfinite(b); }

unsigned grid_y(int64_t items) { return (unsigned)(items < 65535 ? items : 65535); }

}  // namespace

extern "C" {

int femfct_smooth_cost(femfct_ctx* ctx, const double* c_dev, int32_t num_steps, double dt, double* out_host,
                       int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->structured && ctx->d_Ad, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, c_dev && out_host, "null argument");
    ARG_TRY(ctx, num_steps >= 1, "num_steps must be >= 1");
    ARG_TRY(ctx, batch >= 1, "batch must be >= 1");
    ARG_TRY(ctx, dt > 0.0 && std::isfinite(dt), "dt must be finite and > 0");
    const int levels = num_steps + 1;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const int64_t items = (int64_t)levels * batch;
    const size_t plen = (size_t)items * G;
    int rc = femfct_ensure_scratch(ctx, 2 * plen + 2 * (size_t)batch);
    if (rc != FEMFCT_OK) return rc;
    double *part_x = ctx->d_scratch, *part_t = part_x + plen, *res = part_t + plen;
    g.grid.y = grid_y(items);
    hipLaunchKernelGGL(k_smooth_cost_part, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->d_cols, ctx->d_Ad, ctx->d_M, c_dev,
                       levels, items, part_x, part_t);
    // R_x: the trapezoid over the levels times dt; R_t: the plain sum (the last level's partials are 0) times 1 / dt
    femfct_enqueue_reduce_levels(ctx, batch, levels, G, part_x, 1, dt, 0, res);
    femfct_enqueue_reduce_levels(ctx, batch, levels, G, part_t, 0, 1.0 / dt, 0, res + batch);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> host(2 * (size_t)batch);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), res, sizeof(double) * 2 * batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < batch; ++b) {
        out_host[2 * b] = host[b];
        out_host[2 * b + 1] = host[(size_t)batch + b];
    }
    return FEMFCT_OK;
}

int femfct_smooth_rhs(femfct_ctx* ctx, const double* c_dev, double beta_x, double beta_t, int32_t num_steps, double dt,
                      double* out_dev, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->structured && ctx->d_Ad, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, c_dev && out_dev, "null argument");
    ARG_TRY(ctx, num_steps >= 1, "num_steps must be >= 1");
    ARG_TRY(ctx, batch >= 1, "batch must be >= 1");
    ARG_TRY(ctx, dt > 0.0 && std::isfinite(dt), "dt must be finite and > 0");
    ARG_TRY(ctx, coefficient_ok(beta_x), "beta_x must be finite and >= 0");
    ARG_TRY(ctx, coefficient_ok(beta_t), "beta_t must be finite and >= 0");
    const int levels = num_steps + 1;
    const int64_t items = (int64_t)levels * batch;
    LaunchGeom g = femfct_geom(ctx, 1);
    g.grid.y = grid_y(items);
    hipLaunchKernelGGL(k_smooth_rhs, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->d_cols, ctx->d_Ad, ctx->d_M, c_dev, levels,
                       items, beta_x, beta_t, 1.0 / (dt * dt), out_dev);
    HIP_TRY(ctx, hipGetLastError());
    return FEMFCT_OK;
}

int femfct_drift_gradient_rhs_smooth(femfct_ctx* ctx, const double* c_dev, const double* u_dev, const double* p_dev,
                                     double beta, double beta_x, double beta_t, double dt, double* out_dev, int32_t levels,
                                     double bx, double by) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->structured && ctx->d_Ad, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, c_dev && u_dev && p_dev && out_dev, "null argument");
    ARG_TRY(ctx, levels >= 2, "num_steps must be >= 1 (levels >= 2)");
    ARG_TRY(ctx, dt > 0.0 && std::isfinite(dt), "dt must be finite and > 0");
    ARG_TRY(ctx, coefficient_ok(beta_x), "beta_x must be finite and >= 0");
    ARG_TRY(ctx, coefficient_ok(beta_t), "beta_t must be finite and >= 0");
    LaunchGeom g = femfct_geom(ctx, 1);
    g.grid.y = grid_y(levels);
    hipLaunchKernelGGL(k_drift_gradient_rhs_smooth, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->N, ctx->n_cells, ctx->h,
                       ctx->d_d2v, ctx->d_cols, ctx->d_M, ctx->d_Ad, c_dev, u_dev, p_dev, (int)levels, beta, beta_x, beta_t,
                       1.0 / (dt * dt), (beta_x != 0.0 || beta_t != 0.0) ? 1 : 0, bx, by, out_dev);
    HIP_TRY(ctx, hipGetLastError());
    return FEMFCT_OK;
}

}  // extern "C"
