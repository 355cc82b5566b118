// State bounds lo <= u_n <= hi as a Moreau-Yosida penalty on top of snapshot tracking (kernels_obs.hip):
//   v_n = u_n - clip(u_n, lo, hi)                      the nodal violation, signed
//   P   = gamma/2 sum_n sigma_n sum_i ml_i ws_i v_{n,i}^2
// with the lumped mass ml (the max acts node by node), level weights sigma_n >= 0 and an optional nodal window ws >= 0.
// The discrete adjoint of the backward-Euler step for J + P loads the step to level n with the snapshot load minus
// (sigma_n/dt) gamma ml .* ws .* v_n and ends in p_Nt = tau omega (uhat_Nt - u_Nt) - sigma_Nt gamma ws .* v_Nt (nodal, as
// the tracking terminal condition).
//
//   k_bound_load      out = [k_obs_load's row] - (sigma[level]/dt) gamma ml ws v: the load launch of an adjoint step, theta
//                     and sigma read through the device-side level counter.  The tracking and reaction part is
//                     OBS_LOAD_ROW (obs_load_device.h), k_obs_load's expression: v = 0 leaves its bits.  sigma[level] == 0
//                     or gamma == 0: no term, u is not read for the penalty (k_obs_load's bits, the sign of a zero too);
//                     theta[level] == 0: the target is not read.  A NaN in a penalised u gives a NaN load.
//   k_bound_terminal  p_Nt, tau == 0: the target is not read; sigma_Nt == 0 or gamma == 0: u_Nt is not read for the penalty
//   k_bound_cost_part / k_bound_cost_finish   per batch member P, max |v| and the number of v != 0 over the penalised
//                     (level, node) pairs (sigma_n != 0 and ws_i != 0): per-block partials on a grid that depends on n
//                     only, then one finishing block -- a fixed order, the same bits at every batch size.
// One thread per row, no atomics; the penalty is nodal, so it needs no gather and holds in either DoF ordering.
#include "femfct_internal.h"
#include "device_utils.h"
#include "stencil.h"
#include "forms.h"
#include "obs_device.h"
#include "obs_load_device.h"

#include <algorithm>
#include <cmath>

namespace {

// the nodal violation of the bounds, signed.  min / max drop a NaN operand, so a NaN in u stays one in u - clip(u)
// (a compare-and-select form would map it to 0)
__device__ __forceinline__ double bound_violation(double u, double lo, double hi) { return u - fmin(fmax(u, lo), hi); }
__device__ __forceinline__ double bound_lo(const double* lo, int i) { return lo ? lo[i] : -INFINITY; }
__device__ __forceinline__ double bound_hi(const double* hi, int i) { return hi ? hi[i] : INFINITY; }

__global__ void k_bound_load(MeshArgs m, ObsLoadSpec sp, BoundSpec bs, double* __restrict__ out_) {
    const int bz = blockIdx.y, n = m.n;
    const double th = *vec_ptr(sp.theta);       // the level's weights: one value each for the whole grid
    const double sg = *vec_ptr(bs.sigma);
    const double scale = th / sp.dt;
    const double pscale = (sg / sp.dt) * bs.gamma;
    const bool observed = th != 0.0, penalised = pscale != 0.0;     // sigma = 0 or gamma = 0: no term, u unread
    const double* a = observed ? obs_member(sp.a, sp.a_bs, bz) : nullptr;
    const double* b = observed ? obs_member(sp.b, sp.b_bs, bz) : nullptr;
    const double* w = vec_ptr(sp.w);
    const double* g = obs_member(sp.g, 0, bz);
    const double* x = obs_member(sp.x, sp.x_bs, bz);
    const double* u = penalised ? obs_member(bs.u, bs.u_bs, bz) : nullptr;
    double* out = out_ + (int64_t)bz * n;
    const double k60 = 0.5 * m.h * m.h / 60.0;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        OBS_LOAD_ROW(acc)       // reads m, n, i, k60, observed, scale, a, b, w, g, x by name (obs_load_device.h)
        if (penalised) {
            const double v = bound_violation(u[i], bound_lo(bs.lo, i), bound_hi(bs.hi, i));
            double t = pscale * bs.ml[i];
            if (bs.ws) t = t * bs.ws[i];
            acc = acc - t * v;
        }
        out[i] = acc;
    }
}

__global__ void k_bound_terminal(int n, double tau, const double* __restrict__ w, const double* __restrict__ uhat,
                                 int64_t uhat_bs, const double* __restrict__ u, int64_t u_bs,
                                 const double* __restrict__ sigma, double gamma, const double* __restrict__ lo,
                                 const double* __restrict__ hi, const double* __restrict__ ws, double* __restrict__ p,
                                 int64_t p_bs) {
    const int bz = blockIdx.y;
    const double* hb = tau != 0.0 ? uhat + bz * uhat_bs : nullptr;
    const double* ub = u + bz * u_bs;
    const double pscale = *sigma * gamma;
    const bool penalised = pscale != 0.0;       // sigma_Nt = 0 or gamma = 0: u_Nt is not read for the penalty
    double* pb = p + bz * p_bs;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double acc = 0.0;
        if (hb) {
            const double d = hb[i] - ub[i];
            acc = tau * (w ? w[i] * d : d);
        }
        if (penalised) {
            const double v = bound_violation(ub[i], bound_lo(lo, i), bound_hi(hi, i));
            acc = acc - (ws ? pscale * ws[i] : pscale) * v;
        }
        pb[i] = acc;
    }
}

// part[(bz * gridDim.x + blockIdx.x) * 3 + {0, 1, 2}] = over the block's rows and the penalised levels:
// sum sigma_n ml_i ws_i v^2, max |v|, number of v != 0
__global__ void __launch_bounds__(256) k_bound_cost_part(int n, const double* __restrict__ u_, int64_t tstride,
                                                         const double* __restrict__ sigma, const double* __restrict__ lo,
                                                         const double* __restrict__ hi, const double* __restrict__ ml,
                                                         const double* __restrict__ ws, int levels,
                                                         double* __restrict__ part) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    RowRange rr = block_rows(n);
    double sum = 0.0, vmax = 0.0, cnt = 0.0;
    for (int lvl = 0; lvl < levels; ++lvl) {
        const double sg = sigma[lvl];
        if (sg == 0.0) continue;                // uniform: a level without a penalty is not read
        const double* u = u_ + bz * tstride + (int64_t)lvl * n;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double wi = ws ? ws[i] : 1.0;
            if (wi == 0.0) continue;
            const double v = bound_violation(u[i], bound_lo(lo, i), bound_hi(hi, i));
            sum += sg * ((ml[i] * wi) * (v * v));
            vmax = nan_max(vmax, fabs(v));
            if (v != 0.0) cnt += 1.0;
        }
    }
    sum = block_reduce(sum, OpSum(), 0.0, smem);
    vmax = block_reduce(vmax, OpMax(), 0.0, smem);
    cnt = block_reduce(cnt, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) {
        double* o = part + ((int64_t)bz * gridDim.x + blockIdx.x) * 3;
        o[0] = sum; o[1] = vmax; o[2] = cnt;
    }
}

// out[3 b + {0, 1, 2}] = P, max |v|, count of member b from its `count` partial triples
__global__ void __launch_bounds__(256) k_bound_cost_finish(const double* __restrict__ part, int count, int batch, double gamma,
                                                           double* __restrict__ out) {
    __shared__ double smem[32];
    for (int b = 0; b < batch; ++b) {
        const double* pb = part + (int64_t)b * count * 3;
        double s = 0.0, mx = 0.0, c = 0.0;
        for (int k = threadIdx.x; k < count; k += blockDim.x) {
            s += pb[3 * k];
            mx = nan_max(mx, pb[3 * k + 1]);
            c += pb[3 * k + 2];
        }
        s = block_reduce(s, OpSum(), 0.0, smem);
        mx = block_reduce(mx, OpMax(), 0.0, smem);
        c = block_reduce(c, OpSum(), 0.0, smem);
        if (threadIdx.x == 0) {
            out[3 * b] = (0.5 * gamma) * s;
            out[3 * b + 1] = mx;
            out[3 * b + 2] = c;
        }
    }
}

}  // namespace

int femfct_enqueue_bound_load(femfct_ctx* ctx, const ObsLoadSpec& sp, const BoundSpec& bs, double* out, int32_t batch) {
    LaunchGeom g = femfct_geom(ctx, batch);
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_bound_load, g.grid, g.block, 0, ctx->stream, femfct_mesh_args(ctx), sp, bs, out);
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

int femfct_enqueue_bound_terminal(femfct_ctx* ctx, double tau, const double* window, const double* uhat, int64_t uhat_bs,
                                  const double* u, int64_t u_bs, const double* sigma, double gamma, const double* lo,
                                  const double* hi, const double* ws, double* p, int64_t p_bs, int32_t batch) {
    const int bs = 256;
    int64_t g = ((int64_t)ctx->n + bs - 1) / bs;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_bound_terminal, dim3((unsigned)g, (unsigned)batch), dim3(bs), 0, ctx->stream, ctx->n, tau, window, uhat,
                       uhat_bs, u, u_bs, sigma, gamma, lo, hi, ws, p, p_bs);
    return FEMFCT_OK;
}

extern "C" {

int femfct_bound_load(femfct_ctx* ctx, const double* uhat_dev, const double* u_dev, const double* theta_dev,
                      const double* sigma_dev, int32_t level, double dt, const double* window_dev, const double* g_dev,
                      const double* x_dev, const double* lower_dev, const double* upper_dev, double gamma,
                      const double* window_s_dev, double* out_dev, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, theta_dev, "theta is null");
    ARG_TRY(ctx, sigma_dev, "sigma is null");
    ARG_TRY(ctx, lower_dev || upper_dev, "no bound: lower and upper are both null");
    ARG_TRY(ctx, gamma >= 0.0 && std::isfinite(gamma), "gamma must be finite and >= 0");
    ARG_TRY(ctx, !g_dev == !x_dev, "g and x go together");
    ARG_TRY(ctx, uhat_dev && u_dev && out_dev && level >= 0 && dt > 0 && batch >= 1 && batch <= 65535, "bad argument");
    ObsLoadSpec sp;
    sp.a = make_ref(uhat_dev); sp.a_bs = ctx->n;
    sp.b = make_ref(u_dev);    sp.b_bs = ctx->n;
    sp.theta = make_ref(theta_dev + level);
    sp.w = make_ref(window_dev);
    sp.g = make_ref(g_dev);
    sp.x = make_ref(x_dev);    sp.x_bs = ctx->n;
    sp.dt = dt;
    BoundSpec bs;
    bs.sigma = make_ref(sigma_dev + level);
    bs.u = make_ref(u_dev);    bs.u_bs = ctx->n;
    bs.lo = lower_dev; bs.hi = upper_dev; bs.ml = ctx->d_ml; bs.ws = window_s_dev;
    bs.gamma = gamma;
    femfct_enqueue_bound_load(ctx, sp, bs, out_dev, batch);
    HIP_TRY(ctx, hipGetLastError());
    return FEMFCT_OK;
}

int femfct_bound_cost(femfct_ctx* ctx, const double* u_traj, const double* sigma_dev, const double* lower_dev,
                      const double* upper_dev, double gamma, const double* window_s_dev, int32_t num_steps, int32_t batch,
                      double* out_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, sigma_dev, "sigma is null");
    ARG_TRY(ctx, lower_dev || upper_dev, "no bound: lower and upper are both null");
    ARG_TRY(ctx, gamma >= 0.0 && std::isfinite(gamma), "gamma must be finite and >= 0");
    ARG_TRY(ctx, u_traj && out_host && num_steps >= 1 && batch >= 1 && batch <= 65535, "bad argument");
    // the grid depends on n alone: a member's partials, and so its statistics, are the same bits at every batch size
    const int blocks = (int)std::min<int64_t>(1024, ((int64_t)ctx->n + 255) / 256);
    double* d_ws = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_ws, sizeof(double) * 3 * ((size_t)blocks + 1) * batch));
    double* d_out = d_ws + (size_t)3 * blocks * batch;
    hipLaunchKernelGGL(k_bound_cost_part, dim3(blocks, batch), dim3(256), 0, ctx->stream, ctx->n, u_traj,
                       (int64_t)(num_steps + 1) * ctx->n, sigma_dev, lower_dev, upper_dev, ctx->d_ml, window_s_dev,
                       num_steps + 1, d_ws);
    hipLaunchKernelGGL(k_bound_cost_finish, dim3(1), dim3(256), 0, ctx->stream, d_ws, blocks, batch, gamma, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_out, sizeof(double) * 3 * batch, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d_ws);
    HIP_TRY(ctx, e);
    return FEMFCT_OK;
}

}  // extern "C"
