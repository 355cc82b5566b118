// Device primitives of the proximal-gradient loops for L1-sparse controls (solvers.prox_solidbody,
// solvers.prox_source_control; an extension, no reference call):
//   femfct_prox_trials          the K Armijo trial controls c_t = clip(soft_threshold(c + s_t d, s_t alpha)), and their sources
//   femfct_l1_norm_Q            the nodal-quadrature L1(Q) norm dt sum_l w_l sum_i ml_i |a_{l,i}|
//   femfct_sparse_trial_stats   per trial, in one pass: that norm, ||c_t - c||^2_Q and the number of nonzero values
// so that an iteration of the loops moves only scalars across PCIe.
//
// The sums run in k_quadform's fixed tree (per-thread row sums -> wave64 butterflies -> LDS -> per-block partials -> level
// fold by k_reduce_levels, no atomics): bitwise reproducible, and the fused statistics are femfct_l1_norm_Q and
// femfct_l2_norm_sq_Q bit for bit.
#include "femfct_internal.h"
#include "device_utils.h"
#include "prox_device.h"      // prox_value

namespace {

// V neighbouring doubles moved as one access: 16 bytes for V = 2
template <int V> struct Pack { double v[V]; };
template <int V>
__device__ __forceinline__ Pack<V> load_pack(const double* p) {
    Pack<V> r;
    if constexpr (V == 2) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V>
__device__ __forceinline__ void store_pack(double* p, const Pack<V>& a) {
    if constexpr (V == 2) *reinterpret_cast<double2*>(p) = make_double2(a.v[0], a.v[1]);
    else *p = a.v[0];
}

// c_out[t*count + k] = prox_value(c[k], s_t, d[k], s_t alpha), s_t = s0 * (1 / 2^t), src_out[t*count + k] = 1.0*g[k] + 1.0*c_t
// (g NULL: c_t; src_out NULL: no sources), t < K.  V = 2: every thread moves two neighbouring values with 16-byte
// accesses (count even and every pointer 16-byte aligned, so that each trial's block is too); V = 1: any count.
template <int V>
__global__ void __launch_bounds__(256) k_prox_trials(int64_t count, int K, const double* __restrict__ c,
                                                     const double* __restrict__ d, const double* __restrict__ g, double s0,
                                                     double alpha, double lo, double hi, double* __restrict__ c_out,
                                                     double* __restrict__ src_out) {
    const int64_t items = count / V, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < items; q += stride) {
        const int64_t k = q * V;
        const Pack<V> cv = load_pack<V>(c + k), dv = load_pack<V>(d + k);
        Pack<V> gv = cv;
        if (g) gv = load_pack<V>(g + k);
        for (int t = 0; t < K; ++t) {
            const double s = s0 * (1.0 / (double)(1 << t));
            const double tau = s * alpha;
            Pack<V> pv, sv;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                pv.v[e] = prox_value(cv.v[e], s, dv.v[e], tau, lo, hi);
                sv.v[e] = g ? 1.0 * gv.v[e] + 1.0 * pv.v[e] : pv.v[e];
            }
            const int64_t o = (int64_t)t * count + k;
            store_pack<V>(c_out + o, pv);
            if (src_out) store_pack<V>(src_out + o, sv);
        }
    }
}

// partial[q*G + block] = sum_{i in block rows} ml_i |a_{q,i}| for the items q = b*levels + l (a batch member's levels are
// contiguous), strided over gridDim.y (no 65535 cap); k_quadform's row partition and tree, from 0.0
__global__ void __launch_bounds__(256) k_l1_partials(int n, const double* __restrict__ ml, const double* __restrict__ a,
                                                     int64_t items, double* __restrict__ partial) {
    __shared__ double smem[32];
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const double* al = a + q * n;
        double s = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) s += ml[i] * fabs(al[i]);
        s = block_reduce(s, OpSum(), 0.0, smem);
        if (threadIdx.x == 0) partial[q * gridDim.x + blockIdx.x] = s;
    }
}

// Statistics of the K trial controls c_t (K trajectories) against the reference control c (one), one pass: for every item
// q = t*levels + l (strided over gridDim.y) and block
//   part_l[q*G + block]   k_l1_partials' partial of c_t
//   part_d[q*G + block]   k_quadform's partial of phi = c_t - c
//   part_n[q*G + block]   the number of the block's rows with c_t != 0 (exact)
// Rows, expressions and order are those kernels' (block_rows partition, diagonal slot then slots 1..W-1, block_reduce from
// 0.0), so k_reduce_levels over the first two gives femfct_l1_norm_Q's and femfct_l2_norm_sq_Q's bits.  The count of a
// wave is the population count of a ballot: a scalar, no tree.
__global__ void __launch_bounds__(256) k_sparse_trial_stats(int n, int W, const int32_t* __restrict__ cols,
                                                            const double* __restrict__ M, const double* __restrict__ ml,
                                                            const double* __restrict__ ct, const double* __restrict__ c,
                                                            int levels, int64_t items, double* __restrict__ part_l,
                                                            double* __restrict__ part_d,
                                                            unsigned long long* __restrict__ part_n) {
    __shared__ double smem[2 * 4];      // 2 sums x up to 4 waves (blockDim <= 256)
    __shared__ unsigned scnt[4];
    const int G = gridDim.x;
    const int nw = (blockDim.x + WAVE - 1) / WAVE, wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int lvl = (int)(q % levels);
        const double* tl = ct + q * n;
        const double* cl = c + (int64_t)lvl * n;
        double sl = 0.0, sd = 0.0;
        unsigned cnt = 0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double ti = tl[i];
            const double pi = ti - cl[i];
            double acc = M[i] * pi;
            for (int k = 1; k < W; ++k) {
                const int64_t idx = (int64_t)k * n + i;
                const int j = cols[idx];
                acc += M[idx] * (tl[j] - cl[j]);
            }
            sd += pi * acc;
            sl += ml[i] * fabs(ti);
            cnt += (unsigned)__popcll(__ballot(ti != 0.0));
        }
        // the two sums through block_reduce itself, as k_l1_partials and k_quadform reduce theirs (NaN rule included)
        sl = block_reduce(sl, OpSum(), 0.0, smem);
        sd = block_reduce(sd, OpSum(), 0.0, smem + 4);
        if (nw > 1) {
            __syncthreads();   // scnt reuse across items
            if (lane == 0) scnt[wid] = cnt;
            __syncthreads();
            cnt = 0;
            for (int w = 0; w < nw; ++w) cnt += scnt[w];
        }
        if (threadIdx.x == 0) {
            const int64_t pl = q * G + blockIdx.x;
            part_l[pl] = sl;
            part_d[pl] = sd;
            part_n[pl] = cnt;
        }
    }
}

// out[t] = sum of the levels * G counts of trial t (integers: any order gives the same value)
__global__ void __launch_bounds__(256) k_count_fold(int64_t per_trial, const unsigned long long* __restrict__ part,
                                                    unsigned long long* __restrict__ out) {
    __shared__ unsigned long long smem[256];
    const unsigned long long* p = part + (int64_t)blockIdx.x * per_trial;
    unsigned long long s = 0;
    for (int64_t k = threadIdx.x; k < per_trial; k += blockDim.x) s += p[k];
    smem[threadIdx.x] = s;
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) smem[threadIdx.x] += smem[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = smem[0];
}

unsigned grid_y(int64_t work) { return (unsigned)(work < 65535 ? work : 65535); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int femfct_prox_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0, int32_t K,
                       double alpha, double c_lower, double c_upper, int64_t count, double* c_out_dev, double* src_out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, c_dev && d_dev && c_out_dev, "null argument");
    ARG_TRY(ctx, count > 0, "count must be > 0");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_TRIALS, "K (number of Armijo trials) must be in 1..16");
    ARG_TRY(ctx, alpha >= 0.0, "alpha (L1 weight) must be >= 0");
    ARG_TRY(ctx, c_lower <= c_upper, "c_lower must be <= c_upper");
    const bool vec = count % 2 == 0 && aligned16(c_dev) && aligned16(d_dev) && aligned16(g_dev) && aligned16(c_out_dev) &&
                     aligned16(src_out_dev);
    const int bs = 256;
    int64_t gr = (count / (vec ? 2 : 1) + bs - 1) / bs;
    if (gr > 4096) gr = 4096;
    if (gr < 1) gr = 1;
    if (vec)
        hipLaunchKernelGGL(k_prox_trials<2>, dim3((unsigned)gr), dim3(bs), 0, ctx->stream, count, (int)K, c_dev, d_dev, g_dev,
                           s0, alpha, c_lower, c_upper, c_out_dev, src_out_dev);
    else
        hipLaunchKernelGGL(k_prox_trials<1>, dim3((unsigned)gr), dim3(bs), 0, ctx->stream, count, (int)K, c_dev, d_dev, g_dev,
                           s0, alpha, c_lower, c_upper, c_out_dev, src_out_dev);
    return FEMFCT_OK;
}

int femfct_l1_norm_Q(femfct_ctx* ctx, const double* a_dev, int32_t num_steps, double dt, double* out_host, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, a_dev && out_host && num_steps >= 0 && batch >= 1, "bad argument");
    const int levels = num_steps + 1;
    const int64_t items = (int64_t)levels * batch;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t psz = (size_t)items * G;
    int rc = femfct_ensure_scratch(ctx, psz + batch);
    if (rc != FEMFCT_OK) return rc;
    double *part = ctx->d_scratch, *out_dev = part + psz;
    g.grid.y = grid_y(items);
    hipLaunchKernelGGL(k_l1_partials, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->d_ml, a_dev, items, part);
    femfct_enqueue_reduce_levels(ctx, batch, levels, G, part, 1, dt, 0, out_dev);
    HIP_TRY(ctx, hipMemcpyAsync(out_host, out_dev, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FEMFCT_OK;
}

int femfct_sparse_trial_stats(femfct_ctx* ctx, const double* c_trials_dev, const double* c_ref_dev, int32_t K,
                              int32_t num_steps, double dt, double* l1_host, double* dist_host, int64_t* nnz_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, c_trials_dev && c_ref_dev && l1_host && dist_host && nnz_host, "null argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_TRIALS, "K (number of Armijo trials) must be in 1..16");
    ARG_TRY(ctx, num_steps >= 0, "num_steps must be >= 0");
    const int levels = num_steps + 1;
    const int64_t items = (int64_t)levels * K;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    const size_t psz = (size_t)items * G;
    int rc = femfct_ensure_scratch(ctx, 3 * psz + 3 * (size_t)K);
    if (rc != FEMFCT_OK) return rc;
    double *pl = ctx->d_scratch, *pd = pl + psz;
    unsigned long long* pn = reinterpret_cast<unsigned long long*>(pd + psz);      // (8 bytes each, as the doubles)
    double *l1 = pd + 2 * psz, *dist = l1 + K;
    unsigned long long* nnz = reinterpret_cast<unsigned long long*>(dist + K);
    g.grid.y = grid_y(items);
    hipLaunchKernelGGL(k_sparse_trial_stats, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, ctx->d_ml,
                       c_trials_dev, c_ref_dev, levels, items, pl, pd, pn);
    // the level folds of femfct_l1_norm_Q and femfct_l2_norm_sq_Q
    femfct_enqueue_reduce_levels(ctx, K, levels, G, pl, 1, dt, 0, l1);
    femfct_enqueue_reduce_levels(ctx, K, levels, G, pd, 1, dt, 0, dist);
    hipLaunchKernelGGL(k_count_fold, dim3(K), dim3(256), 0, ctx->stream, (int64_t)levels * G, pn, nnz);
    unsigned long long counts[FEMFCT_MAX_TRIALS];
    HIP_TRY(ctx, hipMemcpyAsync(l1_host, l1, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dist_host, dist, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(counts, nnz, sizeof(unsigned long long) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < K; ++t) nnz_host[t] = (int64_t)counts[t];
    return FEMFCT_OK;
}

}  // extern "C"
