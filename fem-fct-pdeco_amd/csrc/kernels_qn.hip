// Device primitives of the limited-memory quasi-Newton loops (solvers.LimitedMemory; an extension, no reference call):
//   femfct_free_set    the free set of a box-constrained control, one byte per value
//   femfct_q_gram      the L2(Q) Gram matrix of up to FEMFCT_MAX_GRAM_FIELDS trajectories, masked to the free set
//   femfct_q_combine   a linear combination of the trajectories on the free set, a scaled fallback field on the bound set
// A direction of any memory is these three launches and one read-back of J*J doubles: the two-loop recursion runs on the
// host on coefficient vectors over the stored fields.
//
// The Gram entries are quadratic forms summed with k_quadform's fixed tree (per-thread row sums -> wave64 butterflies ->
// LDS -> per-block partials -> level fold, no atomics): bitwise reproducible, and the unmasked diagonal is
// femfct_l2_norm_sq_Q bit for bit.
#include "femfct_internal.h"
#include "device_utils.h"

#define QN_TJ 4                                     // columns of G per block: M f_j of QN_TJ fields stay in registers
#define QN_J FEMFCT_MAX_GRAM_FIELDS

namespace {

// device pointers / coefficients of the fields, passed by value in the kernel arguments (as MemberTable in kernels_pgd.hip)
struct FieldTable { const double* p[QN_J]; };
struct CoefTable { double v[QN_J]; };

__global__ void k_free_set(int64_t count, const double* __restrict__ c, const double* __restrict__ g, double lo, double hi,
                           uint8_t* __restrict__ mask) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < count; k += stride) {
        const double ck = c[k], gk = g[k];
        mask[k] = ((ck <= lo && gk > 0.0) || (ck >= hi && gk < 0.0)) ? 0 : 1;
    }
}

__global__ void k_q_combine(int64_t count, FieldTable F, CoefTable coef, int J, const uint8_t* __restrict__ mask,
                            const double* __restrict__ fallback, double fallback_scale, double* __restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < count; k += stride) {
        if (mask && !mask[k]) {
            out[k] = fallback_scale * fallback[k];
            continue;
        }
        double acc = coef.v[0] * F.p[0][k];
        for (int j = 1; j < J; ++j) acc = acc + coef.v[j] * F.p[j][k];
        out[k] = acc;
    }
}

// index of the pair i <= j among the J (J + 1) / 2 entries of the upper triangle, column by column
__host__ __device__ __forceinline__ int tri(int i, int j) { return j * (j + 1) / 2 + i; }

// part[(tri(i, j) * levels + l) * G + block] = sum_{rows of the block} (chi f_i)_row (M chi f_j)_row at level l, for the
// columns j of this block's tile (blockIdx.z * QN_TJ ..) and every i <= j.  Rows, expressions and order are k_quadform's
// (block_rows partition, diagonal slot then slots 1..W-1, the same wave64 / LDS tree; chi f = f - 0.0 = f without a mask),
// so k_gram_fold over these partials gives femfct_l2_norm_sq_Q's bits on the diagonal.  A row reads the stencil of the
// tile's QN_TJ fields and its own value of every f_i once.  Levels are strided over gridDim.y (no 65535 cap).
template <bool MASKED>
__global__ void __launch_bounds__(256) k_q_gram(int n, int W, const int32_t* __restrict__ cols,
                                                const double* __restrict__ M, FieldTable F, int J,
                                                const uint8_t* __restrict__ mask, int levels,
                                                double* __restrict__ part) {
    __shared__ double smem[QN_J * QN_TJ * 4];       // every sum x up to 4 waves (blockDim <= 256)
    const int G = gridDim.x;
    const int nw = (blockDim.x + WAVE - 1) / WAVE, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int jb = blockIdx.z * QN_TJ;              // first column of the tile (uniform over the block)
    const double* fj[QN_TJ];
#pragma unroll
    for (int q = 0; q < QN_TJ; ++q) fj[q] = F.p[jb + q < J ? jb + q : J - 1];
    RowRange rr = block_rows(n);
    for (int lvl = blockIdx.y; lvl < levels; lvl += gridDim.y) {
        const int64_t off = (int64_t)lvl * n;
        const uint8_t* ml = MASKED ? mask + off : nullptr;
        double s[QN_J][QN_TJ];
#pragma unroll
        for (int i = 0; i < QN_J; ++i)
#pragma unroll
            for (int q = 0; q < QN_TJ; ++q) s[i][q] = 0.0;
        for (int r = rr.begin + threadIdx.x; r < rr.end; r += blockDim.x) {
            const double mi = M[r];
            const bool fr = MASKED ? ml[r] != 0 : true;
            double acc[QN_TJ];
#pragma unroll
            for (int q = 0; q < QN_TJ; ++q) acc[q] = mi * (fr ? fj[q][off + r] : 0.0);
            for (int k = 1; k < W; ++k) {
                const int64_t idx = (int64_t)k * n + r;
                const int c = cols[idx];
                const double mk = M[idx];
                const bool fc = MASKED ? ml[c] != 0 : true;
#pragma unroll
                for (int q = 0; q < QN_TJ; ++q) acc[q] += mk * (fc ? fj[q][off + c] : 0.0);
            }
#pragma unroll
            for (int i = 0; i < QN_J; ++i) {
                if (i < J && i < jb + QN_TJ) {      // uniform
                    const double vi = fr ? F.p[i][off + r] : 0.0;
#pragma unroll
                    for (int q = 0; q < QN_TJ; ++q)
                        if (i <= jb + q) s[i][q] += vi * acc[q];
                }
            }
        }
        // block_reduce's tree for each sum: wave butterflies, then the waves in order from 0.0
        if (nw > 1) __syncthreads();   // smem reuse across levels
#pragma unroll
        for (int i = 0; i < QN_J; ++i)
#pragma unroll
            for (int q = 0; q < QN_TJ; ++q)
                if (i <= jb + q && jb + q < J) {    // uniform
                    s[i][q] = wave_reduce(s[i][q], OpSum());
                    if (nw > 1 && lane == 0) smem[(i * QN_TJ + q) * 4 + wid] = s[i][q];
                }
        if (nw > 1) __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < QN_J; ++i)
#pragma unroll
                for (int q = 0; q < QN_TJ; ++q)
                    if (i <= jb + q && jb + q < J) {
                        double v = s[i][q];
                        if (nw > 1) {
                            v = 0.0;
                            for (int w = 0; w < nw; ++w) v = v + smem[(i * QN_TJ + q) * 4 + w];
                        }
                        part[((int64_t)tri(i, jb + q) * levels + lvl) * G + blockIdx.x] = v;
                    }
        }
    }
}

// k_reduce_levels (kernels_pgd.hip) with the trapezoid's weights: out[b] = 0.0 + scale * sum_l w_l sum_blocks partial
__global__ void k_gram_fold(int levels, int G, const double* __restrict__ partial, double scale, double* __restrict__ out) {
    __shared__ double smem[32];
    const int b = blockIdx.x;
    const double* p = partial + (int64_t)b * levels * G;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < (int64_t)levels * G; k += blockDim.x) {
        int l = (int)(k / G);
        double w = (l == 0 || l == levels - 1) ? 0.5 : 1.0;
        s += w * p[k];
    }
    s = block_reduce(s, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) out[b] = 0.0 + scale * s;
}

unsigned pointwise_grid(int64_t count) {
    int64_t g = (count + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// the J pointers of a call, checked, as a table whose unused entries repeat the first field
int field_table(femfct_ctx* ctx, const double* const* fields_host, int32_t J, FieldTable* t) {
    ARG_TRY(ctx, fields_host, "null argument");
    ARG_TRY(ctx, J >= 1 && J <= FEMFCT_MAX_GRAM_FIELDS, "J (number of fields) must be in 1..17");
    for (int j = 0; j < J; ++j) ARG_TRY(ctx, fields_host[j], "null field pointer");
    for (int j = 0; j < QN_J; ++j) t->p[j] = fields_host[j < J ? j : 0];
    return FEMFCT_OK;
}

}  // namespace

extern "C" {

int femfct_free_set(femfct_ctx* ctx, const double* c_dev, const double* g_dev, double c_lower, double c_upper, int64_t count,
                    uint8_t* mask_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, c_dev && g_dev && mask_dev && count >= 0, "bad argument");
    hipLaunchKernelGGL(k_free_set, dim3(pointwise_grid(count)), dim3(256), 0, ctx->stream, count, c_dev, g_dev, c_lower,
                       c_upper, mask_dev);
    return FEMFCT_OK;
}

int femfct_q_gram(femfct_ctx* ctx, const double* const* fields_host, int32_t J, const uint8_t* mask_dev, int32_t num_steps,
                  double dt, double* G_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, G_host && num_steps >= 0, "bad argument");
    FieldTable F;
    int rc = field_table(ctx, fields_host, J, &F);
    if (rc != FEMFCT_OK) return rc;
    const int levels = num_steps + 1, pairs = J * (J + 1) / 2;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t psz = (size_t)pairs * levels * G;
    rc = femfct_ensure_scratch(ctx, psz + pairs);
    if (rc != FEMFCT_OK) return rc;
    double *part = ctx->d_scratch, *out = part + psz;
    g.grid.y = (unsigned)(levels < 65535 ? levels : 65535);
    g.grid.z = (unsigned)((J + QN_TJ - 1) / QN_TJ);
    if (mask_dev)
        hipLaunchKernelGGL(k_q_gram<true>, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, F, (int)J,
                           mask_dev, levels, part);
    else
        hipLaunchKernelGGL(k_q_gram<false>, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, F, (int)J,
                           mask_dev, levels, part);
    hipLaunchKernelGGL(k_gram_fold, dim3(pairs), dim3(256), 0, ctx->stream, levels, G, part, dt, out);
    double upper[QN_J * (QN_J + 1) / 2];
    HIP_TRY(ctx, hipMemcpyAsync(upper, out, sizeof(double) * pairs, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < J; ++j)
        for (int i = 0; i <= j; ++i) G_host[i * J + j] = G_host[j * J + i] = upper[tri(i, j)];
    return FEMFCT_OK;
}

int femfct_q_combine(femfct_ctx* ctx, const double* const* fields_host, const double* coef_host, int32_t J,
                     const uint8_t* mask_dev, const double* fallback_dev, double fallback_scale, int64_t count,
                     double* out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, coef_host && out_dev && count >= 0, "bad argument");
    ARG_TRY(ctx, !mask_dev || fallback_dev, "a mask needs a fallback field");
    FieldTable F;
    int rc = field_table(ctx, fields_host, J, &F);
    if (rc != FEMFCT_OK) return rc;
    CoefTable coef;
    memset(&coef, 0, sizeof(coef));
    memcpy(coef.v, coef_host, sizeof(double) * (size_t)J);
    hipLaunchKernelGGL(k_q_combine, dim3(pointwise_grid(count)), dim3(256), 0, ctx->stream, count, F, coef, (int)J, mask_dev,
                       fallback_dev, fallback_scale, out_dev);
    return FEMFCT_OK;
}

}  // extern "C"
