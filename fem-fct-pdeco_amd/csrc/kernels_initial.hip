// Device primitives of the initial-state recovery (solvers.initial_state_solidbody; an extension, no reference call): the
// control c is fixed and the initial state v = u_0 is the unknown,
//   J(v) = T(u(v)) + beta0/2 (v - v_b)^T M (v - v_b),      g = beta0 (v - v_b) - p_0   (the L2(Omega) representative).
//   femfct_initial_trials        clip(v + s_k dir) written into level 0 of member k of a batch of K trajectories
//   femfct_initial_trial_stats   ||v_k - v_b||^2_M and ||v_k - v||^2_M of every member's level 0, one read-back
//   femfct_initial_gradient      g from level 0 of the adjoint trajectory, with the free set of femfct_free_set on request
//   femfct_omega_gram            the masked L2(Omega) Gram matrix of up to FEMFCT_MAX_GRAM_FIELDS one-level fields
// Every field here is one level of n values: the kernels are latency-sized at n = 1681 / 6561 (the members and the Gram
// tiles are the grid's y / z extent, one launch whatever K or J is) and stream beyond.
//
// No atomics.  The quadratic forms run in k_quadform's fixed tree (kernels_pgd.hip: block_rows partition, diagonal slot
// then slots 1..W-1, per-thread row sums -> wave64 butterflies -> LDS -> per-block partials) and are folded by
// k_reduce_levels with one level, as femfct_l2_norm_sq_Omega folds its own: the statistics and the unmasked Gram diagonal
// are that call's bits.  The pointwise expressions have no contraction (-ffp-contract=off).
#include "femfct_internal.h"
#include "device_utils.h"

#include <cmath>
#include <cstring>

#define IN_TJ 4                                    // columns of G per block (kernels_qn.hip's QN_TJ)
#define IN_J FEMFCT_MAX_GRAM_FIELDS

namespace {

// by value in the kernel arguments (as MemberTable in kernels_pgd.hip, FieldTable in kernels_qn.hip)
struct StepTable { double v[FEMFCT_MAX_MEMBERS]; };
struct FieldTable { const double* p[IN_J]; };

// level 0 of member blockIdx.y: u[k * tstride + i] = clip(v_i + s_k dir_i); k_clip_axpy's expression
__global__ void k_initial_trials(int n, const double* __restrict__ v, const double* __restrict__ dir, StepTable steps,
                                 double lo, double hi, int64_t tstride, double* __restrict__ u) {
    const double s = steps.v[blockIdx.y];
    double* out = u + (int64_t)blockIdx.y * tstride;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = fmin(fmax(v[i] + s * dir[i], lo), hi);
}

// part[((2 k + q) * G + block]: k_quadform's partial of phi = v_k - v_b (q = 0; v_b NULL: v_k - 0.0, as
// femfct_l2_norm_sq_Omega(v_k, NULL) forms it) and of phi = v_k - v (q = 1), v_k = level 0 of member k = blockIdx.y, read
// once for both.  A member's sums see that member alone.
__global__ void k_initial_stats_part(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ M,
                                     const double* __restrict__ u, int64_t tstride, const double* __restrict__ v,
                                     const double* __restrict__ vb, double* __restrict__ part) {
    __shared__ double smem[2 * 32];
    const int k = blockIdx.y;
    const double* a = u + (int64_t)k * tstride;
    RowRange rr = block_rows(n);
    double sb = 0.0, sd = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        const double ai = a[i];
        const double pb = ai - (vb ? vb[i] : 0.0), pd = ai - v[i];
        double ab = M[i] * pb, ad = M[i] * pd;
        for (int s = 1; s < W; ++s) {
            const int64_t idx = (int64_t)s * n + i;
            const int j = cols[idx];
            const double mk = M[idx], aj = a[j];
            ab += mk * (aj - (vb ? vb[j] : 0.0));
            ad += mk * (aj - v[j]);
        }
        sb += pb * ab;
        sd += pd * ad;
    }
    sb = block_reduce(sb, OpSum(), 0.0, smem);
    sd = block_reduce(sd, OpSum(), 0.0, smem + 32);
    if (threadIdx.x == 0) {
        part[((int64_t)2 * k) * gridDim.x + blockIdx.x] = sb;
        part[((int64_t)2 * k + 1) * gridDim.x + blockIdx.x] = sd;
    }
}

// g_i = beta0 (v_i - vb_i) - p_i (vb NULL: v_i - 0.0), p = level 0 of the adjoint trajectory; with mask, k_free_set's
// predicate on (v_i, g_i): the byte femfct_free_set would write from the stored g
__global__ void k_initial_gradient(int n, const double* __restrict__ p, const double* __restrict__ v,
                                   const double* __restrict__ vb, double beta0, double lo, double hi,
                                   double* __restrict__ g, uint8_t* __restrict__ mask) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double vi = v[i];
        const double gi = beta0 * (vi - (vb ? vb[i] : 0.0)) - p[i];
        g[i] = gi;
        if (mask) mask[i] = ((vi <= lo && gi > 0.0) || (vi >= hi && gi < 0.0)) ? 0 : 1;
    }
}

// index of the pair i <= j among the J (J + 1) / 2 entries of the upper triangle, column by column
__host__ __device__ __forceinline__ int tri(int i, int j) { return j * (j + 1) / 2 + i; }

// k_q_gram (kernels_qn.hip) for one level: part[tri(i, j) * G + block] = sum over the block's rows of
// (chi f_i)_row (M chi f_j)_row for the columns j of this block's tile (blockIdx.z * IN_TJ ..) and every i <= j.  Rows,
// expressions and order are k_quadform's, so the fold gives femfct_l2_norm_sq_Omega's bits on the unmasked diagonal.  A
// masked-out value is not read.
template <bool MASKED>
__global__ void __launch_bounds__(256) k_omega_gram(int n, int W, const int32_t* __restrict__ cols,
                                                    const double* __restrict__ M, FieldTable F, int J,
                                                    const uint8_t* __restrict__ mask, double* __restrict__ part) {
    __shared__ double smem[IN_J * IN_TJ * 4];       // every sum x up to 4 waves (blockDim <= 256)
    const int G = gridDim.x;
    const int nw = (blockDim.x + WAVE - 1) / WAVE, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int jb = blockIdx.z * IN_TJ;              // first column of the tile (uniform over the block)
    const double* fj[IN_TJ];
#pragma unroll
    for (int q = 0; q < IN_TJ; ++q) fj[q] = F.p[jb + q < J ? jb + q : J - 1];
    RowRange rr = block_rows(n);
    double s[IN_J][IN_TJ];
#pragma unroll
    for (int i = 0; i < IN_J; ++i)
#pragma unroll
        for (int q = 0; q < IN_TJ; ++q) s[i][q] = 0.0;
    for (int r = rr.begin + threadIdx.x; r < rr.end; r += blockDim.x) {
        const double mi = M[r];
        const bool fr = MASKED ? mask[r] != 0 : true;
        double acc[IN_TJ];
#pragma unroll
        for (int q = 0; q < IN_TJ; ++q) acc[q] = mi * (fr ? fj[q][r] : 0.0);
        for (int k = 1; k < W; ++k) {
            const int64_t idx = (int64_t)k * n + r;
            const int c = cols[idx];
            const double mk = M[idx];
            const bool fc = MASKED ? mask[c] != 0 : true;
#pragma unroll
            for (int q = 0; q < IN_TJ; ++q) acc[q] += mk * (fc ? fj[q][c] : 0.0);
        }
#pragma unroll
        for (int i = 0; i < IN_J; ++i) {
            if (i < J && i < jb + IN_TJ) {          // uniform
                const double vi = fr ? F.p[i][r] : 0.0;
#pragma unroll
                for (int q = 0; q < IN_TJ; ++q)
                    if (i <= jb + q) s[i][q] += vi * acc[q];
            }
        }
    }
    // block_reduce's tree for each sum: wave butterflies, then the waves in order from 0.0
#pragma unroll
    for (int i = 0; i < IN_J; ++i)
#pragma unroll
        for (int q = 0; q < IN_TJ; ++q)
            if (i <= jb + q && jb + q < J) {        // uniform
                s[i][q] = wave_reduce(s[i][q], OpSum());
                if (nw > 1 && lane == 0) smem[(i * IN_TJ + q) * 4 + wid] = s[i][q];
            }
    if (nw > 1) __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < IN_J; ++i)
#pragma unroll
            for (int q = 0; q < IN_TJ; ++q)
                if (i <= jb + q && jb + q < J) {
                    double v = s[i][q];
                    if (nw > 1) {
                        v = 0.0;
                        for (int w = 0; w < nw; ++w) v = v + smem[(i * IN_TJ + q) * 4 + w];
                    }
                    part[(int64_t)tri(i, jb + q) * G + blockIdx.x] = v;
                }
    }
}

unsigned pointwise_grid(int n) {
    int g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

extern "C" {

int femfct_initial_trials(femfct_ctx* ctx, const double* v_dev, const double* dir_dev, const double* steps_host, int32_t K,
                          double v_lower, double v_upper, double* u_traj_dev, int32_t num_steps) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0, "mesh not set");
    ARG_TRY(ctx, v_dev && dir_dev && steps_host && u_traj_dev, "null argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_MEMBERS, "K (trial members) must be in 1..256");
    ARG_TRY(ctx, num_steps >= 0, "num_steps must be >= 0");
    ARG_TRY(ctx, v_lower <= v_upper, "v_lower must be <= v_upper");
    StepTable steps;
    memset(&steps, 0, sizeof(steps));
    memcpy(steps.v, steps_host, sizeof(double) * (size_t)K);
    hipLaunchKernelGGL(k_initial_trials, dim3(pointwise_grid(ctx->n), (unsigned)K), dim3(256), 0, ctx->stream, ctx->n, v_dev,
                       dir_dev, steps, v_lower, v_upper, ((int64_t)num_steps + 1) * ctx->n, u_traj_dev);
    return FEMFCT_OK;
}

int femfct_initial_trial_stats(femfct_ctx* ctx, const double* u_traj_dev, const double* v_dev, const double* vb_dev,
                               int32_t K, int32_t num_steps, double* out_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, u_traj_dev && v_dev && out_host, "null argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_MEMBERS, "K (trial members) must be in 1..256");
    ARG_TRY(ctx, num_steps >= 0, "num_steps must be >= 0");
    LaunchGeom g = femfct_geom(ctx, K);             // femfct_l2_norm_sq_Omega's row partition and block, members along y
    const int G = g.grid.x;
    const size_t psz = (size_t)2 * K * G;
    int rc = femfct_ensure_scratch(ctx, psz + 2 * (size_t)K);
    if (rc != FEMFCT_OK) return rc;
    double *part = ctx->d_scratch, *out = part + psz;
    hipLaunchKernelGGL(k_initial_stats_part, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M,
                       u_traj_dev, ((int64_t)num_steps + 1) * ctx->n, v_dev, vb_dev, part);
    femfct_enqueue_reduce_levels(ctx, 2 * K, 1, G, part, 0, 1.0, 0, out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_host, out, sizeof(double) * 2 * (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_initial_gradient(femfct_ctx* ctx, const double* p_traj_dev, const double* v_dev, const double* vb_dev,
                            double beta0, double* g_dev, double v_lower, double v_upper, uint8_t* mask_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0, "mesh not set");
    ARG_TRY(ctx, p_traj_dev && v_dev && g_dev, "null argument");
    ARG_TRY(ctx, beta0 >= 0.0 && std::isfinite(beta0), "beta0 must be finite and >= 0");
    ARG_TRY(ctx, !mask_dev || v_lower <= v_upper, "v_lower must be <= v_upper");
    hipLaunchKernelGGL(k_initial_gradient, dim3(pointwise_grid(ctx->n)), dim3(256), 0, ctx->stream, ctx->n, p_traj_dev,
                       v_dev, vb_dev, beta0, v_lower, v_upper, g_dev, mask_dev);
    return FEMFCT_OK;
}

int femfct_omega_gram(femfct_ctx* ctx, const double* const* fields_host, int32_t J, const uint8_t* mask_dev,
                      double* G_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, fields_host && G_host, "null argument");
    ARG_TRY(ctx, J >= 1 && J <= FEMFCT_MAX_GRAM_FIELDS, "J (number of fields) must be in 1..17");
    FieldTable F;
    for (int j = 0; j < J; ++j) ARG_TRY(ctx, fields_host[j], "null field pointer");
    for (int j = 0; j < IN_J; ++j) F.p[j] = fields_host[j < J ? j : 0];
    const int pairs = J * (J + 1) / 2;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t psz = (size_t)pairs * G;
    int rc = femfct_ensure_scratch(ctx, psz + pairs);
    if (rc != FEMFCT_OK) return rc;
    double *part = ctx->d_scratch, *out = part + psz;
    g.grid.z = (unsigned)((J + IN_TJ - 1) / IN_TJ);
    if (mask_dev)
        hipLaunchKernelGGL(k_omega_gram<true>, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, F,
                           (int)J, mask_dev, part);
    else
        hipLaunchKernelGGL(k_omega_gram<false>, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, F,
                           (int)J, mask_dev, part);
    femfct_enqueue_reduce_levels(ctx, pairs, 1, G, part, 0, 1.0, 0, out);
    HIP_TRY(ctx, hipGetLastError());
    double upper[IN_J * (IN_J + 1) / 2];
    HIP_TRY(ctx, hipMemcpyAsync(upper, out, sizeof(double) * pairs, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < J; ++j)
        for (int i = 0; i <= j; ++i) G_host[i * J + j] = G_host[j * J + i] = upper[tri(i, j)];
    return FEMFCT_OK;
}

}  // extern "C"
