// Row-strip multi-sweep kernels (temporal blocking) for any ELL pattern: k_strip_jacobi, k_strip_cheb.  Selected by
// femfct_strip_plan (end of this file) where the 2-D kernels of the structured mesh (kernels_tile32.hip,
// kernels_patch64.hip) do not apply.
//
// On the config meshes (n = 1681 / 6561) a Jacobi sweep or a Chebyshev step moves < 1 MB and costs
// one dependent kernel boundary (~2.7 us measured) -- the step is launch-latency bound, not
// bandwidth bound.  These kernels run K sweeps per launch: a 1024-thread workgroup owns R
// consecutive rows, stages the iterate for its rows plus a halo of K*bw rows (bw = matrix
// bandwidth, N+1 on the structured mesh in either DoF order) in LDS, keeps its matrix rows
// (values + LDS-local column offsets) in registers, and sweeps K times with __syncthreads()
// between sweeps; the region of valid rows shrinks by bw per sweep and still covers the owned rows
// at the end.  Arithmetic per row is identical to the one-sweep kernels (same operation order),
// nothing is exchanged between workgroups inside a launch, no atomics: deterministic.
// Works for any ELL pattern whose bandwidth admits K >= 2 within the LDS/register budget.
#include "femfct_internal.h"
#include "device_utils.h"
#include "solve_ctl.h"
#include "sweep_common.h"

#include <math.h>

namespace {

template <int RPT>
__global__ void __launch_bounds__(STRIP_T)
k_strip_jacobi(int n, const int32_t* __restrict__ cols, const double* __restrict__ L_, const double* __restrict__ b_,
               double* __restrict__ xa_, double* __restrict__ xb_, double* __restrict__ part,
               StepCtl* __restrict__ ctl_, int launch, int K, int bw, int R, int g_build, double rel_tol) {
    constexpr int W = 7, EXT = RPT * STRIP_T;
    extern __shared__ double lds[];
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    StepCtl* ctl = ctl_ + bz;
    if (ctl->done) return;
    double* p = part + (int64_t)bz * 4 * FEMFCT_MAX_PARTIALS;
    double bnorm;
    if (launch == 0) {
        bnorm = reduce_partials(p + 2 * FEMFCT_MAX_PARTIALS, g_build, OpMax(), 0.0, smem);
        double rsmin = reduce_partials(p + 3 * FEMFCT_MAX_PARTIALS, g_build, OpMin(), INFINITY, smem);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ctl->bnorm = bnorm;
            ctl->min_rowsum = rsmin;
            if (!(rsmin > 0.0)) ctl->flags |= FEMFCT_FLAG_MMATRIX_ROWSUM;
        }
    } else {
        bnorm = ctl->bnorm;
        double rmax = reduce_partials(p + ((launch - 1) & 1) * FEMFCT_MAX_PARTIALS, gridDim.x, OpMax(), 0.0, smem);
        if (rmax <= rel_tol * bnorm) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                ctl->done = 1; ctl->parity = launch & 1; ctl->iters = launch * K; ctl->flags |= FEMFCT_FLAG_COARSE_ITERS;
                ctl->resid = bnorm != 0.0 ? rmax / bnorm : 0.0;
            }
            return;
        }
    }
    const int64_t moff = (int64_t)bz * W * n, voff = (int64_t)bz * n;
    const double* L = L_ + moff;
    const double* b = b_ + voff;
    const double* xin = ((launch & 1) ? xb_ : xa_) + voff;
    double* xout = ((launch & 1) ? xa_ : xb_) + voff;

    const int r0 = blockIdx.x * R, r1 = min(n, r0 + R);
    const int e0 = max(0, r0 - K * bw), e1 = min(n, r1 + K * bw), ext = e1 - e0;
    double lv[RPT][W];       // lv[r][0] holds 1 / L_ii after loading
    double dg[RPT];
    int lc[RPT][W - 1];
    double bv[RPT];
    double* cur = lds;
    double* nxt = lds + EXT;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int li = threadIdx.x + r * STRIP_T;
        if (li < ext) {
            const int i = e0 + li;
            dg[r] = L[i];
            lv[r][0] = 1.0 / dg[r];
#pragma unroll
            for (int s = 1; s < W; ++s) {
                int64_t idx = (int64_t)s * n + i;
                lv[r][s] = L[idx];
                int c = cols[idx] - e0;
                lc[r][s - 1] = (c >= 0 && c < ext) ? c : li;
            }
            bv[r] = b[i];
            cur[li] = xin[i];
        }
    }
    __syncthreads();
    double rmax = 0.0;
    for (int k = 0; k < K; ++k) {
        const int lo = (e0 == 0) ? 0 : (k + 1) * bw;
        const int hi = (e1 == n) ? ext : ext - (k + 1) * bw;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int li = threadIdx.x + r * STRIP_T;
            if (li < ext) {
                const double xi = cur[li];
                double xn = xi;
                if (li >= lo && li < hi) {
                    double acc = bv[r];
#pragma unroll
                    for (int s = 1; s < W; ++s) acc = fma(-lv[r][s], cur[lc[r][s - 1]], acc);
                    xn = acc * lv[r][0];          // one reciprocal per row and launch instead of K divisions
                    const int i = e0 + li;
                    if (k == K - 1 && i >= r0 && i < r1) rmax = nan_max(rmax, fabs(acc - dg[r] * xi));
                }
                nxt[li] = xn;
            }
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int li = threadIdx.x + r * STRIP_T;
        const int i = e0 + li;
        if (li < ext && i >= r0 && i < r1) xout[i] = cur[li];
    }
    rmax = block_reduce(rmax, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) p[(launch & 1) * FEMFCT_MAX_PARTIALS + blockIdx.x] = rmax;
}

// Chebyshev semi-iteration steps k0..k1-1 (1-based iteration numbers as in helpers.py:175):
//   y_k = w_k ( (b - M y_{k-1}) / Md + y_{k-1} - y_{k-2} ) + y_{k-2}
// in: y_{k0-1} (mid, null = 0), y_{k0-2} (old, null = 0); out: y_{k1-1} (mid) and y_{k1-2} (old, optional)
template <int RPT>
__global__ void __launch_bounds__(STRIP_T)
k_strip_cheb(int n, const int32_t* __restrict__ cols, const double* __restrict__ M, const double* __restrict__ b_,
             const double* __restrict__ ymid_, const double* __restrict__ yold_, double* __restrict__ omid_,
             double* __restrict__ oold_, int k0, int k1, CheOmegas om, double md_scale, int bw, int R) {
    constexpr int W = 7, EXT = RPT * STRIP_T;
    extern __shared__ double lds[];
    const int64_t voff = (int64_t)blockIdx.y * n;
    const double* b = b_ + voff;
    const double* ymid = ymid_ ? ymid_ + voff : nullptr;
    const double* yold = yold_ ? yold_ + voff : nullptr;
    double* omid = omid_ + voff;
    double* oold = oold_ ? oold_ + voff : nullptr;
    const int K = k1 - k0;
    const int r0 = blockIdx.x * R, r1 = min(n, r0 + R);
    const int e0 = max(0, r0 - K * bw), e1 = min(n, r1 + K * bw), ext = e1 - e0;
    double mv[RPT][W];
    double rmd[RPT];         // 1 / (md_scale * M_ii)
    int lc[RPT][W - 1];
    double bv[RPT];
    double* y_old = lds;
    double* y_mid = lds + EXT;
    double* y_new = lds + 2 * EXT;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int li = threadIdx.x + r * STRIP_T;
        if (li < ext) {
            const int i = e0 + li;
            mv[r][0] = M[i];
#pragma unroll
            for (int s = 1; s < W; ++s) {
                int64_t idx = (int64_t)s * n + i;
                mv[r][s] = M[idx];
                int c = cols[idx] - e0;
                lc[r][s - 1] = (c >= 0 && c < ext) ? c : li;
            }
            bv[r] = b[i];
            rmd[r] = 1.0 / (md_scale * mv[r][0]);
            y_mid[li] = ymid ? ymid[i] : 0.0;
            y_old[li] = yold ? yold[i] : 0.0;
        }
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const int lo = (e0 == 0) ? 0 : (k + 1) * bw;
        const int hi = (e1 == n) ? ext : ext - (k + 1) * bw;
        const double omega = om.w[k];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int li = threadIdx.x + r * STRIP_T;
            if (li < ext) {
                const double ym = y_mid[li];
                double yn = ym;
                if (li >= lo && li < hi) {
                    double acc = mv[r][0] * ym;
#pragma unroll
                    for (int s = 1; s < W; ++s) acc = fma(mv[r][s], y_mid[lc[r][s - 1]], acc);
                    const double rr = bv[r] - acc;
                    const double z = rr * rmd[r];
                    const double yo = y_old[li];
                    yn = omega * (z + ym - yo) + yo;
                }
                y_new[li] = yn;
            }
        }
        __syncthreads();
        double* t = y_old; y_old = y_mid; y_mid = y_new; y_new = t;
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int li = threadIdx.x + r * STRIP_T;
        const int i = e0 + li;
        if (li < ext && i >= r0 && i < r1) {
            omid[i] = y_mid[li];
            if (oold) oold[i] = y_old[li];
        }
    }
}

}  // namespace

int femfct_strip_init(femfct_ctx* ctx) {
    // > 64 KB of dynamic LDS needs the attribute
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_strip_cheb<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * STRIP_T * 8));
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_strip_cheb<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 4 * STRIP_T * 8));
    return femfct_tile4_init(ctx);
}

int femfct_enqueue_strip_jacobi(femfct_ctx* ctx, const StripPlan& pl, const double* L, const double* b, double* xa,
                                double* xb, int launch, int g_build, int32_t batch) {
    dim3 grid(pl.S, batch, 1);
    size_t lds = (size_t)2 * pl.rpt * STRIP_T * 8;
    femfct_prof_begin(ctx, KC_JACOBI);
    with_constant<2, 4>(pl.rpt, [&](auto rpt) {
        hipLaunchKernelGGL((k_strip_jacobi<decltype(rpt)::value>), grid, dim3(STRIP_T), lds, ctx->stream, ctx->n, ctx->d_cols, L,
                           b, xa, xb, ctx->d_part, ctx->d_ctl, launch, pl.K, pl.bw, pl.R, g_build, ctx->rel_tol);
    });
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

int femfct_enqueue_strip_cheb(femfct_ctx* ctx, const StripPlan& pl, const double* b, const double* in_mid,
                              const double* in_old, double* y_out, int k_first, int k_last, const double* omegas,
                              double md_scale, double* bufA0, double* bufA1, double* bufB0, double* bufB1,
                              int32_t batch) {
    dim3 grid(pl.S, batch, 1);
    size_t lds = (size_t)3 * pl.rpt * STRIP_T * 8;
    for_cheb_launches(k_first, k_last, pl.K, omegas, in_mid, in_old, y_out, bufA0, bufA1, bufB0, bufB1,
                      [&](int k0, int k1, const CheOmegas& om, const double* mid, const double* old, double* omid, double* oold) {
        femfct_prof_begin(ctx, KC_CHEB);
        with_constant<2, 4>(pl.rpt, [&](auto rpt) {
            hipLaunchKernelGGL((k_strip_cheb<decltype(rpt)::value>), grid, dim3(STRIP_T), lds, ctx->stream, ctx->n, ctx->d_cols,
                               ctx->d_M, b, mid, old, omid, oold, k0, k1, om, md_scale, pl.bw, pl.R);
        });
        femfct_prof_end(ctx);
    });
    return FEMFCT_OK;
}

// ---- policy: when the row strips run ---------------------------------------------------------------

// Plan: K sweeps per launch, R owned rows per workgroup, RPT rows per thread.  Returns false when
// the pattern's bandwidth leaves no room for K >= 2 (large meshes: the bandwidth-bound kernels win).
bool femfct_strip_plan(const femfct_ctx* ctx, StripPlan* pl) {
    if (!ctx->use_strips || ctx->W != 7 || ctx->bandwidth <= 0) return false;
    const int bw = ctx->bandwidth;
    int K = 1300 / bw;
    if (K > 8) K = 8;
    if (ctx->strip_k > 0) K = std::min(ctx->strip_k, 1800 / bw);   // tuning knob (FEMFCT_STRIP_K)
    if (K > 8) K = 8;
    if (K < 2) return false;
    const int halo = K * bw;
    // fewest rows per thread that still leave >= 256 owned rows, then the largest R for that
    int rpt = (2 * halo + 256 + STRIP_T - 1) / STRIP_T;
    if (rpt < 2) rpt = 2;
    if (rpt > 4) return false;
    int R = rpt * STRIP_T - 2 * halo;
    if (R > ctx->n) R = ctx->n;
    pl->K = K; pl->R = R; pl->bw = bw; pl->rpt = rpt;
    pl->S = (ctx->n + R - 1) / R;
    return true;
}
