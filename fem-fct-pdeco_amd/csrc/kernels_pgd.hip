// Optimisation-layer reductions and updates kept on the device so that a projected
// gradient iteration moves only scalars across PCIe:
//   L2_norm_sq_Q / L2_norm_sq_Omega   /root/reference/helpers.py:330-381
//   cost_functional                   /root/reference/helpers.py:383-441
//   update_control (clip)             /root/reference/helpers.py:1666-1667
//   Armijo trial batches              helpers.py:1681-1708, advection_FCT_PDECO_alltime_exact.py:282-297
//
// Quadratic forms phi^T M phi are summed with a fixed reduction tree (per-thread row
// sums -> wave64 butterflies -> LDS -> per-block partials -> one block), no atomics:
// bitwise reproducible.
#include "femfct_internal.h"
#include "device_utils.h"

#include <utility>

namespace {

// partial[level*G + block] = sum_{i in block rows} phi_i (M phi)_i,  phi = a - b
__global__ void k_quadform(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ M,
                           const double* __restrict__ a_, const double* __restrict__ b_, int64_t a_lstride,
                           int64_t b_lstride, double* __restrict__ partial) {
    __shared__ double smem[32];
    const int lvl = blockIdx.y;
    const double* a = a_ + (int64_t)lvl * a_lstride;
    const double* b = b_ ? b_ + (int64_t)lvl * b_lstride : nullptr;
    RowRange rr = block_rows(n);
    double s = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double pi = a[i] - (b ? b[i] : 0.0);
        double acc = M[i] * pi;
        for (int k = 1; k < W; ++k) {
            int64_t idx = (int64_t)k * n + i;
            int j = cols[idx];
            acc += M[idx] * (a[j] - (b ? b[j] : 0.0));
        }
        s += pi * acc;
    }
    s = block_reduce(s, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) partial[(int64_t)lvl * gridDim.x + blockIdx.x] = s;
}

// out[b] (+)= scale * sum_l w_l * sum_blocks partial[(b*levels + l)*G + block]
// w_l = 1 except 1/2 at the first and last level when trapezoid != 0.
__global__ void k_reduce_levels(int levels, int G, const double* __restrict__ partial, int trapezoid, double scale,
                                int accumulate, double* __restrict__ out) {
    __shared__ double smem[32];
    const int b = blockIdx.x;
    const double* p = partial + (int64_t)b * levels * G;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < (int64_t)levels * G; k += blockDim.x) {
        int l = (int)(k / G);
        double w = (trapezoid && (l == 0 || l == levels - 1)) ? 0.5 : 1.0;
        s += w * p[k];
    }
    s = block_reduce(s, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) out[b] = (accumulate ? out[b] : 0.0) + scale * s;
}

// (out may alias c -- femfct.h: neither is __restrict__)
__global__ void k_clip_axpy(int64_t count, const double* c, double s, const double* __restrict__ d, double lo, double hi,
                            double* out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < count; k += stride) out[k] = fmin(fmax(c[k] + s * d[k], lo), hi);
}

// d = -(beta*c - t),  t = x*y/divisor (y given) or scale*x: the pointwise gradient expressions of the
// refactored drivers, evaluated in the reference's operation order (no contraction: -ffp-contract=off)
//   nonlinear_FCT_PDECO_refactored.py:148   dk = -(beta*ck - pk)
//   Schnak_FCT_PDECO_refactored.py:167      dk = -(beta*ck - gamma/rescaling*pk)
//   chemotaxis_FCT_PDECO_AT_refactored.py:158   dk = -(beta*ck - qk*uk/rescaling)
__global__ void k_descent_pointwise(int64_t count, double beta, const double* __restrict__ c, double scale,
                                    const double* __restrict__ x, const double* __restrict__ y, double divisor,
                                    double* __restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < count; k += stride) {
        const double t = y ? (x[k] * y[k]) / divisor : scale * x[k];
        out[k] = -(beta * c[k] - t);
    }
}

// All K Armijo trials of the linear-increment search (advection_FCT_PDECO_alltime_exact.py:282-297, helpers.py:1681-1708)
// in one pass over u, w, uhat, c, d.  Trial t has s_t = s0 * (1 / 2^t), c_t = clip(c + s_t d) and the state u + s_t w;
// for every (level, block) the launch writes the three k_quadform partials the materialised path would compute:
//   misfit   phi = (u + s_t w) - uhat   (every level; level Nt only, against the n-value target, when finaltime)
//   control  phi = c_t - 0.0
//   dist     phi = c_t - c
// Rows, expressions and order are k_quadform's (block_rows partition, diagonal then slots 1..W-1, the same wave64 /
// LDS tree), so k_reduce_levels over these partials gives the bits of femfct_cost_functional / femfct_l2_norm_sq_Q on
// materialised trials.  Levels are strided over gridDim.y (no 65535 cap).  Partials: misfit at [t*plen_m + l*G + blk]
// (plen_m = G when finaltime, l = 0), control / dist at [t*levels*G + l*G + blk].
template <int K>
__global__ void __launch_bounds__(256) k_linear_trials(int n, int W, const int32_t* __restrict__ cols,
                                                       const double* __restrict__ M, const double* __restrict__ u,
                                                       const double* __restrict__ w, const double* __restrict__ uhat,
                                                       const double* __restrict__ c, const double* __restrict__ d,
                                                       double s0, double lo, double hi, int levels, int finaltime,
                                                       double* __restrict__ part_m, double* __restrict__ part_c,
                                                       double* __restrict__ part_d) {
    __shared__ double smem[3 * K * 4];      // 3K sums x up to 4 waves (blockDim <= 256)
    const int G = gridDim.x;
    const int64_t plen = (int64_t)levels * G, plen_m = finaltime ? G : plen;
    const int nw = (blockDim.x + WAVE - 1) / WAVE, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    double s[K];
#pragma unroll
    for (int t = 0; t < K; ++t) s[t] = s0 * (1.0 / (double)(1 << t));
    RowRange rr = block_rows(n);
    for (int lvl = blockIdx.y; lvl < levels; lvl += gridDim.y) {
        const bool mis = !finaltime || lvl == levels - 1;         // uniform over the block
        const int64_t off = (int64_t)lvl * n;
        const double *ul = u + off, *wl = w + off, *cl = c + off, *dl = d + off;
        const double* hl = uhat + (finaltime ? 0 : off);
        double sm[K], sc[K], sd[K];
#pragma unroll
        for (int t = 0; t < K; ++t) sm[t] = sc[t] = sd[t] = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            double am[K], ac[K], ad[K];
            const double mi = M[i], ci = cl[i], di = dl[i];
            const double ui = mis ? ul[i] : 0.0, wi = mis ? wl[i] : 0.0, hi_ = mis ? hl[i] : 0.0;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const double ct = fmin(fmax(ci + s[t] * di, lo), hi);
                am[t] = mi * ((ui + s[t] * wi) - hi_);
                ac[t] = mi * (ct - 0.0);
                ad[t] = mi * (ct - ci);
            }
            for (int k = 1; k < W; ++k) {
                const int64_t idx = (int64_t)k * n + i;
                const int j = cols[idx];
                const double mk = M[idx], cj = cl[j], dj = dl[j];
                const double uj = mis ? ul[j] : 0.0, wj = mis ? wl[j] : 0.0, hj = mis ? hl[j] : 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const double ct = fmin(fmax(cj + s[t] * dj, lo), hi);
                    am[t] += mk * ((uj + s[t] * wj) - hj);
                    ac[t] += mk * (ct - 0.0);
                    ad[t] += mk * (ct - cj);
                }
            }
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const double ct = fmin(fmax(ci + s[t] * di, lo), hi);
                sm[t] += ((ui + s[t] * wi) - hi_) * am[t];
                sc[t] += (ct - 0.0) * ac[t];
                sd[t] += (ct - ci) * ad[t];
            }
        }
        // block_reduce's tree for each of the 3K sums: wave butterflies, then the waves in order from 0.0
#pragma unroll
        for (int t = 0; t < K; ++t) {
            sm[t] = wave_reduce(sm[t], OpSum());
            sc[t] = wave_reduce(sc[t], OpSum());
            sd[t] = wave_reduce(sd[t], OpSum());
        }
        if (nw > 1) {
            __syncthreads();   // smem reuse across levels
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    smem[(3 * t) * 4 + wid] = sm[t];
                    smem[(3 * t + 1) * 4 + wid] = sc[t];
                    smem[(3 * t + 2) * 4 + wid] = sd[t];
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < K; ++t) {
                double rm = 0.0, rc = 0.0, rd = 0.0;
                for (int q = 0; q < nw; ++q) {
                    rm = rm + smem[(3 * t) * 4 + q];
                    rc = rc + smem[(3 * t + 1) * 4 + q];
                    rd = rd + smem[(3 * t + 2) * 4 + q];
                }
                sm[t] = rm; sc[t] = rc; sd[t] = rd;
            }
        }
        if (threadIdx.x == 0) {
            const int64_t pl = (int64_t)lvl * G + blockIdx.x;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                if (mis) part_m[t * plen_m + (finaltime ? blockIdx.x : pl)] = sm[t];
                part_c[t * plen + pl] = sc[t];
                part_d[t * plen + pl] = sd[t];
            }
        }
    }
}

// Resolve-mode trials: c_out[t] = clip(c + s_t d) as k_clip_axpy, src_out[t] = g + c_out[t] as k_axpby(1, g, 1, c_t)
// (g NULL: src_out[t] = c_out[t]; src_out NULL: no sources), t < K, each block member count doubles long.
__global__ void k_source_trials(int64_t count, int K, const double* __restrict__ c, const double* __restrict__ d,
                                const double* __restrict__ g, double s0, double lo, double hi,
                                double* __restrict__ c_out, double* __restrict__ src_out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < count; k += stride) {
        const double ck = c[k], dk = d[k], gk = g ? g[k] : 0.0;
        for (int t = 0; t < K; ++t) {
            const double s = s0 * (1.0 / (double)(1 << t));
            const double ct = fmin(fmax(ck + s * dk, lo), hi);
            c_out[t * count + k] = ct;
            if (src_out) src_out[t * count + k] = g ? 1.0 * gk + 1.0 * ct : ct;
        }
    }
}

// One double per member of a lockstep batch, passed by value in the kernel arguments (2 KiB): no device buffer to own,
// fill or synchronise on.
struct MemberTable { double v[FEMFCT_MAX_MEMBERS]; };

// Lockstep trial controls: member m = p*K + t of P problems x K trials, c_out[m] = clip(c[p] + steps[m] * d[p]) with
// k_clip_axpy's expression; c and d hold P blocks of count doubles (blockIdx.y strides the problems), c_out P*K.
__global__ void k_trial_controls(int64_t count, int P, int K, const double* __restrict__ c, const double* __restrict__ d,
                                 MemberTable steps, double lo, double hi, double* __restrict__ c_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const double *cp = c + (int64_t)p * count, *dp = d + (int64_t)p * count;
        double* op = c_out + (int64_t)p * K * count;
        for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
            const double ck = cp[k], dk = dp[k];
            for (int t = 0; t < K; ++t) op[t * count + k] = fmin(fmax(ck + steps.v[p * K + t] * dk, lo), hi);
        }
    }
}

// Costs of the members of a lockstep batch in one pass: for member m = p*K + t (u_m, c_m its trajectories, uhat_p / cref_p
// its problem's target and reference control) and every (level, block) the three k_quadform partials
//   misfit   phi = u_m - uhat_p    (every level; level Nt only, against the n-value target, when finaltime)
//   control  phi = c_m - 0.0
//   dist     phi = c_m - cref_p    (cref given)
// A row reads its stencil of u_m, uhat_p, c_m, cref_p once and forms the three sums in registers.  Rows, expressions and
// order are k_quadform's (block_rows partition, diagonal then slots 1..W-1, the same wave64 / LDS tree), as in
// k_linear_trials, so the level folds over these partials give the bits of femfct_cost_functional / femfct_l2_norm_sq_Q on
// each member alone.  (member, level) pairs are strided over gridDim.y (no 65535 cap).  Partials: misfit at
// [m*plen_m + l*G + blk] (plen_m = G when finaltime, l = 0), control / dist at [(m*levels + l)*G + blk].
__global__ void __launch_bounds__(256) k_member_costs(int n, int W, const int32_t* __restrict__ cols,
                                                      const double* __restrict__ M, const double* __restrict__ u,
                                                      const double* __restrict__ uhat, int64_t uhat_pstride,
                                                      const double* __restrict__ c, const double* __restrict__ cref,
                                                      int K, int levels, int64_t items, int finaltime,
                                                      double* __restrict__ part_m, double* __restrict__ part_c,
                                                      double* __restrict__ part_d) {
    __shared__ double smem[3 * 4];      // 3 sums x up to 4 waves (blockDim <= 256)
    const int G = gridDim.x;
    const int nw = (blockDim.x + WAVE - 1) / WAVE, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t tl = (int64_t)levels * n;
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int m = (int)(q / levels), lvl = (int)(q % levels), p = m / K;
        const bool mis = !finaltime || lvl == levels - 1;         // uniform over the block
        const int64_t off = (int64_t)lvl * n;
        const double *ul = u + m * tl + off, *cl = c + m * tl + off;
        const double* hl = uhat + p * uhat_pstride + (finaltime ? 0 : off);
        const double* rl = cref ? cref + p * tl + off : nullptr;
        double sm = 0.0, sc = 0.0, sd = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double mi = M[i], ci = cl[i];
            const double pm = mis ? ul[i] - hl[i] : 0.0, pc = ci - 0.0, pd = rl ? ci - rl[i] : 0.0;
            double am = mi * pm, ac = mi * pc, ad = mi * pd;
            for (int k = 1; k < W; ++k) {
                const int64_t idx = (int64_t)k * n + i;
                const int j = cols[idx];
                const double mk = M[idx], cj = cl[j];
                if (mis) am += mk * (ul[j] - hl[j]);
                ac += mk * (cj - 0.0);
                if (rl) ad += mk * (cj - rl[j]);
            }
            sm += pm * am;
            sc += pc * ac;
            sd += pd * ad;
        }
        // block_reduce's tree for each of the three sums: wave butterflies, then the waves in order from 0.0
        sm = wave_reduce(sm, OpSum());
        sc = wave_reduce(sc, OpSum());
        sd = wave_reduce(sd, OpSum());
        if (nw > 1) {
            __syncthreads();   // smem reuse across items
            if (lane == 0) { smem[wid] = sm; smem[4 + wid] = sc; smem[8 + wid] = sd; }
            __syncthreads();
            double rm = 0.0, rc = 0.0, rd = 0.0;
            for (int w = 0; w < nw; ++w) {
                rm = rm + smem[w];
                rc = rc + smem[4 + w];
                rd = rd + smem[8 + w];
            }
            sm = rm; sc = rc; sd = rd;
        }
        if (threadIdx.x == 0) {
            const int64_t pl = q * G + blockIdx.x;
            if (mis) part_m[finaltime ? (int64_t)m * G + blockIdx.x : pl] = sm;
            part_c[pl] = sc;
            if (rl) part_d[pl] = sd;
        }
    }
}

// k_reduce_levels with one scale per batch member (the beta of a member's problem): out[b] (+)= scale.v[b] * sum ...
__global__ void k_reduce_levels_member(int levels, int G, const double* __restrict__ partial, int trapezoid,
                                       MemberTable scale, int accumulate, double* __restrict__ out) {
    __shared__ double smem[32];
    const int b = blockIdx.x;
    const double* p = partial + (int64_t)b * levels * G;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < (int64_t)levels * G; k += blockDim.x) {
        int l = (int)(k / G);
        double w = (trapezoid && (l == 0 || l == levels - 1)) ? 0.5 : 1.0;
        s += w * p[k];
    }
    s = block_reduce(s, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) out[b] = (accumulate ? out[b] : 0.0) + scale.v[b] * s;
}

int ensure_scratch(femfct_ctx* ctx, size_t doubles) {
    if (doubles <= ctx->scratch_count) return FEMFCT_OK;
    if (ctx->d_scratch) hipFree(ctx->d_scratch);
    ctx->d_scratch = nullptr;
    ctx->scratch_count = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_scratch, sizeof(double) * doubles));
    ctx->scratch_count = doubles;
    return FEMFCT_OK;
}

// enqueue: out_dev[b] (+)= scale * sum_levels w phi^T M phi   (phi = a - b)
int enqueue_norm(femfct_ctx* ctx, const double* a, const double* b, int64_t a_lstride, int64_t b_lstride, int levels,
                 int trapezoid, double scale, int accumulate, int32_t batch, double* out_dev, size_t scratch_off) {
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    g.grid.y = (unsigned)(levels * batch);
    double* part = ctx->d_scratch + scratch_off;
    hipLaunchKernelGGL(k_quadform, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, a, b,
                       a_lstride, b_lstride, part);
    femfct_enqueue_reduce_levels(ctx, batch, levels, G, part, trapezoid, scale, accumulate, out_dev);
    return FEMFCT_OK;
}

}  // namespace

int femfct_ensure_scratch(femfct_ctx* ctx, size_t doubles) { return ensure_scratch(ctx, doubles); }

void femfct_enqueue_reduce_levels(femfct_ctx* ctx, int32_t batch, int levels, int G, const double* partial, int trapezoid,
                                  double scale, int accumulate, double* out_dev) {
    hipLaunchKernelGGL(k_reduce_levels, dim3(batch), dim3(256), 0, ctx->stream, levels, G, partial, trapezoid, scale,
                       accumulate, out_dev);
}

extern "C" {

int femfct_l2_norm_sq_Q(femfct_ctx* ctx, const double* a_dev, const double* b_dev, int32_t num_steps, double dt,
                        double* out_host, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, a_dev && out_host && num_steps >= 0 && batch >= 1, "bad argument");
    const int levels = num_steps + 1;
    ARG_TRY(ctx, (int64_t)levels * batch <= 65535, "too many levels*batch for one launch");
    LaunchGeom g = femfct_geom(ctx, 1);
    int rc = ensure_scratch(ctx, (size_t)levels * batch * g.grid.x + batch);
    if (rc != FEMFCT_OK) return rc;
    double* out_dev = ctx->d_scratch + (size_t)levels * batch * g.grid.x;
    // a batch member's levels are contiguous, so (batch, level) flattens to one level index
    enqueue_norm(ctx, a_dev, b_dev, ctx->n, ctx->n, levels, 1, dt, 0, batch, out_dev, 0);
    HIP_TRY(ctx, hipMemcpyAsync(out_host, out_dev, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_l2_norm_sq_Omega(femfct_ctx* ctx, const double* a_dev, const double* b_dev, double* out_host,
                            int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, a_dev && out_host && batch >= 1 && batch <= 65535, "bad argument");
    LaunchGeom g = femfct_geom(ctx, 1);
    int rc = ensure_scratch(ctx, (size_t)batch * g.grid.x + batch);
    if (rc != FEMFCT_OK) return rc;
    double* out_dev = ctx->d_scratch + (size_t)batch * g.grid.x;
    enqueue_norm(ctx, a_dev, b_dev, ctx->n, ctx->n, 1, 0, 1.0, 0, batch, out_dev, 0);
    HIP_TRY(ctx, hipMemcpyAsync(out_host, out_dev, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_cost_functional(femfct_ctx* ctx, const double* var1, const double* var1_target, const double* control,
                           int32_t control_shared, int32_t num_steps, double dt, double beta, int32_t finaltime,
                           const double* var2, const double* var2_target, double* J_host, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, var1 && var1_target && control && J_host && num_steps >= 1 && batch >= 1, "bad argument");
    ARG_TRY(ctx, (var2 == nullptr) == (var2_target == nullptr), "var2 and var2_target must be given together");
    const int levels = num_steps + 1;
    ARG_TRY(ctx, (int64_t)levels * batch <= 65535, "too many levels*batch for one launch");
    LaunchGeom g = femfct_geom(ctx, 1);
    const size_t psz = (size_t)levels * batch * g.grid.x;
    int rc = ensure_scratch(ctx, psz + batch);
    if (rc != FEMFCT_OK) return rc;
    double* J = ctx->d_scratch + psz;
    const int64_t n = ctx->n, tstride = (int64_t)levels * n;
    if (!finaltime) {
        // 0.5 * ||var - target||^2_{L2(Q)}  (helpers.py:422-426)
        enqueue_norm(ctx, var1, var1_target, n, n, levels, 1, 0.5 * dt, 0, batch, J, 0);
        if (var2) enqueue_norm(ctx, var2, var2_target, n, n, levels, 1, 0.5 * dt, 1, batch, J, 0);
    } else {
        // 0.5 * ||var(T) - target||^2_{L2(Omega)}  (helpers.py:428-434): target is n doubles per batch member
        enqueue_norm(ctx, var1 + (int64_t)num_steps * n, var1_target, tstride, n, 1, 0, 0.5, 0, batch, J, 0);
        if (var2) enqueue_norm(ctx, var2 + (int64_t)num_steps * n, var2_target, tstride, n, 1, 0, 0.5, 1, batch, J, 0);
    }
    // + beta/2 ||c||^2_{L2(Q)}  (helpers.py:440)
    if (control_shared) {
        // one control for the whole batch: norm once into a spare slot, then add to every member
        ARG_TRY(ctx, batch == 1, "control_shared requires batch == 1 in femfct_cost_functional");
    }
    enqueue_norm(ctx, control, nullptr, n, n, levels, 1, 0.5 * beta * dt, 1, batch, J, 0);
    HIP_TRY(ctx, hipMemcpyAsync(J_host, J, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_descent_pointwise(femfct_ctx* ctx, int64_t count, double beta, const double* c_dev, double scale,
                             const double* x_dev, const double* y_dev, double divisor, double* out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && c_dev && x_dev && out_dev && count >= 0 && divisor != 0.0, "bad argument");
    int bs = 256;
    int64_t g = (count + bs - 1) / bs;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_descent_pointwise, dim3((unsigned)g), dim3(bs), 0, ctx->stream, count, beta, c_dev, scale, x_dev,
                       y_dev, divisor, out_dev);
    return FEMFCT_OK;
}

int femfct_project_control(femfct_ctx* ctx, const double* c_dev, double s, const double* d_dev, double c_lower,
                           double c_upper, double* out_dev, int64_t count) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && c_dev && d_dev && out_dev && count >= 0, "bad argument");
    int bs = 256;
    int64_t g = (count + bs - 1) / bs;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_clip_axpy, dim3((unsigned)g), dim3(bs), 0, ctx->stream, count, c_dev, s, d_dev, c_lower,
                       c_upper, out_dev);
    return FEMFCT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- Armijo trial batches
namespace {

template <int K>
void launch_linear_trials(dim3 grid, dim3 block, hipStream_t st, int n, int W, const int32_t* cols, const double* M,
                          const double* u, const double* w, const double* uhat, const double* c, const double* d,
                          double s0, double lo, double hi, int levels, int finaltime, double* pm, double* pc, double* pd) {
    hipLaunchKernelGGL(k_linear_trials<K>, grid, block, 0, st, n, W, cols, M, u, w, uhat, c, d, s0, lo, hi, levels,
                       finaltime, pm, pc, pd);
}

using LinearTrialsLaunch = void (*)(dim3, dim3, hipStream_t, int, int, const int32_t*, const double*, const double*,
                                    const double*, const double*, const double*, const double*, double, double, double,
                                    int, int, double*, double*, double*);

template <int... Ks>
constexpr LinearTrialsLaunch linear_trials_table(int K, std::integer_sequence<int, Ks...>) {
    constexpr LinearTrialsLaunch tab[] = {launch_linear_trials<Ks + 1>...};
    return tab[K - 1];
}

}  // namespace

extern "C" {

int femfct_linear_trial_costs(femfct_ctx* ctx, const double* u_dev, const double* w_dev, const double* uhat_dev,
                              const double* c_dev, const double* d_dev, double s0, int32_t K, double c_lower,
                              double c_upper, double beta, int32_t num_steps, double dt, int32_t finaltime,
                              double* J_host, double* dist_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, u_dev && w_dev && uhat_dev && c_dev && d_dev && J_host && dist_host, "null argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_TRIALS, "K (number of Armijo trials) must be in 1..16");
    ARG_TRY(ctx, num_steps >= 1, "num_steps must be >= 1");
    const int levels = num_steps + 1;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t plen = (size_t)levels * G, plen_m = finaltime ? (size_t)G : plen;
    int rc = ensure_scratch(ctx, (size_t)K * (plen_m + 2 * plen) + 2 * (size_t)K);
    if (rc != FEMFCT_OK) return rc;
    double* pm = ctx->d_scratch;
    double* pc = pm + (size_t)K * plen_m;
    double* pd = pc + (size_t)K * plen;
    double* J = pd + (size_t)K * plen;
    double* dist = J + K;
    g.grid.y = (unsigned)(levels < 65535 ? levels : 65535);
    linear_trials_table(K, std::make_integer_sequence<int, FEMFCT_MAX_TRIALS>())(
        g.grid, g.block, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, u_dev, w_dev, uhat_dev, c_dev, d_dev, s0,
        c_lower, c_upper, levels, finaltime, pm, pc, pd);
    // the level reductions and scale / accumulate order of femfct_cost_functional and femfct_l2_norm_sq_Q
    if (!finaltime)
        hipLaunchKernelGGL(k_reduce_levels, dim3(K), dim3(256), 0, ctx->stream, levels, G, pm, 1, 0.5 * dt, 0, J);
    else
        hipLaunchKernelGGL(k_reduce_levels, dim3(K), dim3(256), 0, ctx->stream, 1, G, pm, 0, 0.5, 0, J);
    hipLaunchKernelGGL(k_reduce_levels, dim3(K), dim3(256), 0, ctx->stream, levels, G, pc, 1, 0.5 * beta * dt, 1, J);
    hipLaunchKernelGGL(k_reduce_levels, dim3(K), dim3(256), 0, ctx->stream, levels, G, pd, 1, dt, 0, dist);
    HIP_TRY(ctx, hipMemcpyAsync(J_host, J, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dist_host, dist, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_source_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0,
                         int32_t K, double c_lower, double c_upper, int64_t count, double* c_out_dev,
                         double* src_out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, c_dev && d_dev && c_out_dev && count >= 0, "bad argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_TRIALS, "K (number of Armijo trials) must be in 1..16");
    int bs = 256;
    int64_t gr = (count + bs - 1) / bs;
    if (gr > 4096) gr = 4096;
    if (gr < 1) gr = 1;
    hipLaunchKernelGGL(k_source_trials, dim3((unsigned)gr), dim3(bs), 0, ctx->stream, count, (int)K, c_dev, d_dev, g_dev,
                       s0, c_lower, c_upper, c_out_dev, src_out_dev);
    return FEMFCT_OK;
}

// ------------------------------------------------------------------------ lockstep batches: P problems x K trials
int femfct_trial_controls(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* steps_host, int32_t P,
                          int32_t K, double c_lower, double c_upper, int64_t count, double* c_out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, c_dev && d_dev && steps_host && c_out_dev && count >= 0, "bad argument");
    ARG_TRY(ctx, P >= 1 && K >= 1 && (int64_t)P * K <= FEMFCT_MAX_MEMBERS, "P*K (problems x trials) must be in 1..256");
    MemberTable steps;
    memset(&steps, 0, sizeof(steps));
    memcpy(steps.v, steps_host, sizeof(double) * (size_t)(P * K));
    int bs = 256;
    int64_t gr = (count + bs - 1) / bs;
    if (gr > 4096) gr = 4096;
    if (gr < 1) gr = 1;
    hipLaunchKernelGGL(k_trial_controls, dim3((unsigned)gr, (unsigned)P), dim3(bs), 0, ctx->stream, count, (int)P, (int)K,
                       c_dev, d_dev, steps, c_lower, c_upper, c_out_dev);
    return FEMFCT_OK;
}

int femfct_member_costs(femfct_ctx* ctx, const double* u_traj, const double* uhat, int32_t uhat_per_problem,
                        const double* c_traj, const double* cref, const double* beta_host, int32_t P, int32_t K,
                        int32_t num_steps, double dt, int32_t finaltime, double* J_host, double* dist_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, u_traj && uhat && c_traj && beta_host && J_host, "null argument");
    ARG_TRY(ctx, !cref || dist_host, "cref needs dist_host");
    ARG_TRY(ctx, uhat_per_problem == 0 || uhat_per_problem == 1, "uhat_per_problem must be 0 or 1");
    ARG_TRY(ctx, P >= 1 && K >= 1 && (int64_t)P * K <= FEMFCT_MAX_MEMBERS, "P*K (problems x trials) must be in 1..256");
    ARG_TRY(ctx, num_steps >= 1, "num_steps must be >= 1");
    const int levels = num_steps + 1, members = P * K;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t plen = (size_t)levels * G, plen_m = finaltime ? (size_t)G : plen;
    int rc = ensure_scratch(ctx, (size_t)members * (plen_m + 2 * plen) + 2 * (size_t)members);
    if (rc != FEMFCT_OK) return rc;
    double* pm = ctx->d_scratch;
    double* pc = pm + (size_t)members * plen_m;
    double* pd = pc + (size_t)members * plen;
    double* J = pd + (size_t)members * plen;
    double* dist = J + members;
    const int64_t items = (int64_t)levels * members, tl = (int64_t)levels * ctx->n;
    g.grid.y = (unsigned)(items < 65535 ? items : 65535);
    hipLaunchKernelGGL(k_member_costs, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, u_traj, uhat,
                       uhat_per_problem ? (finaltime ? (int64_t)ctx->n : tl) : (int64_t)0, c_traj, cref, (int)K, levels,
                       items, finaltime, pm, pc, pd);
    // the level reductions and scale / accumulate order of femfct_cost_functional and femfct_l2_norm_sq_Q; the control
    // term's scale 0.5 * beta * dt is formed here per member as femfct_cost_functional forms it
    MemberTable scale;
    memset(&scale, 0, sizeof(scale));
    for (int m = 0; m < members; ++m) scale.v[m] = 0.5 * beta_host[m / K] * dt;
    if (!finaltime)
        hipLaunchKernelGGL(k_reduce_levels, dim3(members), dim3(256), 0, ctx->stream, levels, G, pm, 1, 0.5 * dt, 0, J);
    else
        hipLaunchKernelGGL(k_reduce_levels, dim3(members), dim3(256), 0, ctx->stream, 1, G, pm, 0, 0.5, 0, J);
    hipLaunchKernelGGL(k_reduce_levels_member, dim3(members), dim3(256), 0, ctx->stream, levels, G, pc, 1, scale, 1, J);
    HIP_TRY(ctx, hipMemcpyAsync(J_host, J, sizeof(double) * members, hipMemcpyDeviceToHost, ctx->stream));
    if (cref) {
        hipLaunchKernelGGL(k_reduce_levels, dim3(members), dim3(256), 0, ctx->stream, levels, G, pd, 1, dt, 0, dist);
        HIP_TRY(ctx, hipMemcpyAsync(dist_host, dist, sizeof(double) * members, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------ controls piecewise constant in time
// K intervals of time levels, interval k = the levels starts[k] <= l < starts[k+1] (starts[0] = 0, starts[K] = levels).
// With the trapezoid's level weights w_l (1, and 1/2 at the first and last level; dt cancels) and W_k = sum_{l in k} w_l
//   restrict(x)[k] = (sum_{l in k} w_l x_l) / W_k      one field of n values per interval
//   prolong(y)[l]  = y[k(l)]
// prolong(restrict(.)) is the L2(Q)-orthogonal projection (the inner product of femfct_l2_norm_sq_Q) onto the controls
// that are constant in time on every interval.
//
// k_time_restrict is a column sum: lane = node (unit-stride loads), the levels of an interval are cut into chunks of
// TR_CH, one block each, and a chunk into runs of TR_LW levels, one wave each.  A wave sums its run in level order in a
// register (the TR_LW loads are independent), wave 0 adds the runs of its chunk in order through LDS, and where an
// interval has more than one chunk k_time_restrict_fold adds the chunk sums in order from a partials buffer.  The order
// of an interval's sum depends on its length alone: no atomics, the same bits for every batch size, member and run.  An
// interval of one level gives (w x) / w = x exactly.
#define TR_LW 8
#define TR_CH 32

namespace {

// Device table of a set of intervals (int32): starts[K+1], first work item of interval k [K+1], first partial of
// interval k [K+1] (an interval of one chunk has none), interval of work item j [items], interval of level l [levels].
struct TimeTable { const int32_t *starts, *ifirst, *pfirst, *item_k, *level_k; int K, items, nparts, maxlen; };

__device__ __forceinline__ double trapezoid_w(int l, int levels) { return (l == 0 || l == levels - 1) ? 0.5 : 1.0; }
__device__ __forceinline__ double interval_weight(int s, int e, int levels) {
    return (double)(e - s) - (s == 0 ? 0.5 : 0.0) - (e == levels ? 0.5 : 0.0);
}

// blockDim.x = 256, or 64 when no interval is longer than TR_LW; work = batch * items, strided over gridDim.y
__global__ void __launch_bounds__(256) k_time_restrict(int n, int levels, TimeTable t, int64_t work,
                                                       const double* __restrict__ x, double* __restrict__ out,
                                                       double* __restrict__ part) {
    __shared__ double smem[(TR_CH / TR_LW) * WAVE];
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int i = blockIdx.x * WAVE + lane;
    for (int64_t q = blockIdx.y; q < work; q += gridDim.y) {
        const int64_t b = q / t.items;
        const int it = (int)(q % t.items), k = t.item_k[it], c = it - t.ifirst[k];
        const int s = t.starts[k], e = t.starts[k + 1];
        const int c0 = s + c * TR_CH, c1 = min(c0 + TR_CH, e);      // this block's chunk
        const int used = (c1 - c0 + TR_LW - 1) / TR_LW;              // waves with a run (uniform over the block)
        const int l0 = c0 + wid * TR_LW, l1 = min(l0 + TR_LW, c1);
        double acc = 0.0;
        if (i < n && l0 < l1) {
            const double* xp = x + b * levels * n + i;
            double v[TR_LW];
#pragma unroll
            for (int j = 0; j < TR_LW; ++j) v[j] = l0 + j < l1 ? xp[(int64_t)(l0 + j) * n] : 0.0;
            acc = trapezoid_w(l0, levels) * v[0];
#pragma unroll
            for (int j = 1; j < TR_LW; ++j)
                if (l0 + j < l1) acc += trapezoid_w(l0 + j, levels) * v[j];
        }
        if (used > 1) {
            __syncthreads();   // smem reuse across work items
            smem[wid * WAVE + lane] = acc;
            __syncthreads();
            if (wid == 0) {
                acc = smem[lane];
                for (int w = 1; w < used; ++w) acc += smem[w * WAVE + lane];
            }
        }
        if (wid == 0 && i < n) {
            if (e - s <= TR_CH) out[(b * t.K + k) * n + i] = acc / interval_weight(s, e, levels);
            else part[(b * t.nparts + t.pfirst[k] + c) * n + i] = acc;
        }
    }
}

// the intervals of more than one chunk: out = (chunk sums, added in order) / W_k; work = batch * K over gridDim.y
__global__ void k_time_restrict_fold(int n, int levels, TimeTable t, int64_t work, const double* __restrict__ part,
                                     double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t q = blockIdx.y; q < work; q += gridDim.y) {
        const int64_t b = q / t.K;
        const int k = (int)(q % t.K), s = t.starts[k], e = t.starts[k + 1];
        if (e - s <= TR_CH) continue;
        const int nch = (e - s + TR_CH - 1) / TR_CH;
        const double* p = part + (b * t.nparts + t.pfirst[k]) * n + i;
        double acc = p[0];
        for (int c = 1; c < nch; ++c) acc += p[(int64_t)c * n];
        out[(b * t.K + k) * n + i] = acc / interval_weight(s, e, levels);
    }
}

// out[b][l] = y[b][k(l)]; work = batch * levels over gridDim.y
__global__ void k_time_prolong(int n, int levels, TimeTable t, int64_t work, const double* __restrict__ y,
                               double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t q = blockIdx.y; q < work; q += gridDim.y) {
        const int64_t b = q / levels;
        const int l = (int)(q % levels);
        out[q * n + i] = y[(b * t.K + t.level_k[l]) * n + i];
    }
}

// Checks ``starts`` and makes the intervals' table resident on the device (uploaded when it differs from the one there).
int time_table(femfct_ctx* ctx, const int32_t* starts, int32_t K, int32_t levels, TimeTable* t) {
    ARG_TRY(ctx, starts && K >= 1 && K <= levels, "starts: K + 1 levels with 1 <= K <= num_steps + 1");
    ARG_TRY(ctx, starts[0] == 0 && starts[K] == levels, "starts must begin at 0 and end at num_steps + 1");
    for (int k = 0; k < K; ++k) ARG_TRY(ctx, starts[k] < starts[k + 1], "starts must be strictly increasing");
    std::vector<int32_t> h(starts, starts + K + 1), ifirst(K + 1), pfirst(K + 1), item_k, level_k(levels);
    int items = 0, nparts = 0, maxlen = 0;
    for (int k = 0; k < K; ++k) {
        const int len = starts[k + 1] - starts[k], nch = (len + TR_CH - 1) / TR_CH;
        ifirst[k] = items;
        pfirst[k] = nparts;
        items += nch;
        if (nch > 1) nparts += nch;
        if (len > maxlen) maxlen = len;
        item_k.insert(item_k.end(), nch, k);
        for (int l = starts[k]; l < starts[k + 1]; ++l) level_k[l] = k;
    }
    ifirst[K] = items;
    pfirst[K] = nparts;
    h.insert(h.end(), ifirst.begin(), ifirst.end());
    h.insert(h.end(), pfirst.begin(), pfirst.end());
    h.insert(h.end(), item_k.begin(), item_k.end());
    h.insert(h.end(), level_k.begin(), level_k.end());
    if (h != ctx->h_ttab) {
        if (h.size() > ctx->ttab_count) {
            if (ctx->d_ttab) hipFree(ctx->d_ttab);
            ctx->d_ttab = nullptr;
            ctx->ttab_count = 0;
            ctx->h_ttab.clear();
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_ttab, sizeof(int32_t) * h.size()));
            ctx->ttab_count = h.size();
        }
        ctx->h_ttab.clear();      // (stays empty, and the next call uploads again, should the copy fail)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ttab, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, ctx->stream));
        ctx->h_ttab.swap(h);
    }
    const int32_t* d = ctx->d_ttab;
    *t = TimeTable{d, d + (K + 1), d + 2 * (K + 1), d + 3 * (K + 1), d + 3 * (K + 1) + items, K, items, nparts, maxlen};
    return FEMFCT_OK;
}

unsigned grid_y(int64_t work) { return (unsigned)(work < 65535 ? work : 65535); }

}  // namespace

extern "C" {

int femfct_time_restrict(femfct_ctx* ctx, const double* x_traj, const int32_t* starts_host, int32_t K, int32_t num_steps,
                         int32_t batch, double* out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0, "pattern not set");
    ARG_TRY(ctx, x_traj && out_dev && num_steps >= 1 && batch >= 1, "bad argument");
    const int levels = num_steps + 1, n = ctx->n;
    TimeTable t;
    int rc = time_table(ctx, starts_host, K, levels, &t);
    if (rc != FEMFCT_OK) return rc;
    if (t.nparts) {
        rc = ensure_scratch(ctx, (size_t)batch * t.nparts * n);
        if (rc != FEMFCT_OK) return rc;
    }
    const unsigned tiles = (unsigned)((n + WAVE - 1) / WAVE);
    const int64_t work = (int64_t)batch * t.items;
    hipLaunchKernelGGL(k_time_restrict, dim3(tiles, grid_y(work)), dim3(t.maxlen <= TR_LW ? WAVE : 256), 0, ctx->stream, n,
                       levels, t, work, x_traj, out_dev, ctx->d_scratch);
    if (t.nparts)
        hipLaunchKernelGGL(k_time_restrict_fold, dim3((unsigned)((n + 255) / 256), grid_y((int64_t)batch * K)), dim3(256), 0,
                           ctx->stream, n, levels, t, (int64_t)batch * K, ctx->d_scratch, out_dev);
    return FEMFCT_OK;
}

int femfct_time_prolong(femfct_ctx* ctx, const double* y_dev, const int32_t* starts_host, int32_t K, int32_t num_steps,
                        int32_t batch, double* out_traj) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0, "pattern not set");
    ARG_TRY(ctx, y_dev && out_traj && num_steps >= 1 && batch >= 1, "bad argument");
    const int levels = num_steps + 1, n = ctx->n;
    TimeTable t;
    int rc = time_table(ctx, starts_host, K, levels, &t);
    if (rc != FEMFCT_OK) return rc;
    const int64_t work = (int64_t)batch * levels;
    hipLaunchKernelGGL(k_time_prolong, dim3((unsigned)((n + 255) / 256), grid_y(work)), dim3(256), 0, ctx->stream, n, levels,
                       t, work, y_dev, out_traj);
    return FEMFCT_OK;
}

}  // extern "C"
