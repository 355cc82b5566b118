// Jacobi-preconditioned BiCGStab for the reference's non-FCT implicit solves
//   spsolve(M + dt*(Dv*Ad - w2*A + g*M_u2), ...)   helpers.py:595-596, 685-686   (non-symmetric)
//   spsolve(M + dt*(Df*Ad + delta*M), ...)         helpers.py:1308,1342,1536-1538 (SPD)
//
// Three kernels per iteration; all scalars (rho, alpha, omega, norms) live on the device and are
// obtained by every block re-reducing per-block partial sums in a fixed order (deterministic, no
// atomics, no host round trip).  The vector updates that feed an SpMV are recomputed for the
// neighbour rows inside the SpMV kernel (p_j, s_j), which removes two kernel boundaries per
// iteration at the price of cached gathers.  Convergence (||r||_inf <= tol ||b||_inf) is tested
// on the device; the captured sequence runs a fixed iteration budget that the host adapts.
#include "femfct_internal.h"
#include "device_utils.h"
#include "forms.h"
#include "step_end.h"

#include <float.h>
#include <math.h>

namespace {

struct KryVecs {
    double *x, *r, *rh, *p0, *p1, *v0, *v1, *s, *t;
    double* part;    // [B][6][MAX_PARTIALS]: 0 rho, 1 rh.v, 2 t.s, 3 t.t, 4 |r|max, 5 |b|max
    KrylovCtl* ctl;
};

#define KP(p, k) ((p) + (int64_t)(k) * FEMFCT_MAX_PARTIALS)

__global__ void k_kry_init(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ A_, int ashared,
                           const double* __restrict__ b_, VecRef x0_ref, int64_t x0_bs, KryVecs kv) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    const int64_t voff = (int64_t)bz * n;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    const double* b = b_ + voff;
    const double* x0 = vec_ptr(x0_ref) + bz * x0_bs;
    double *x = kv.x + voff, *r = kv.r + voff, *rh = kv.rh + voff;
    double *p0 = kv.p0 + voff, *v0 = kv.v0 + voff;
    double* part = kv.part + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        KrylovCtl* c = kv.ctl + bz;
        c->flags = 0; c->iters = 0; c->done = 0; c->resid = 0.0; c->bnorm = 0.0;
        c->rho2[0] = 1.0; c->rho2[1] = 1.0; c->alpha = 1.0; c->omega = 1.0;
    }
    RowRange rr = block_rows(n);
    double rho = 0.0, rmax = 0.0, bmax = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double xi = x0[i];
        double acc = A[i] * xi;
        for (int s = 1; s < W; ++s) {
            int64_t idx = (int64_t)s * n + i;
            acc += A[idx] * x0[cols[idx]];
        }
        double bi = b[i];
        double ri = bi - acc;
        x[i] = xi; r[i] = ri; rh[i] = ri; p0[i] = 0.0; v0[i] = 0.0;
        rho += ri * ri;
        rmax = nan_max(rmax, fabs(ri));
        bmax = nan_max(bmax, fabs(bi));
    }
    rho = block_reduce(rho, OpSum(), 0.0, smem);
    rmax = block_reduce(rmax, OpMax(), 0.0, smem);
    bmax = block_reduce(bmax, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) {
        KP(part, 0)[blockIdx.x] = rho;
        KP(part, 4)[blockIdx.x] = rmax;
        KP(part, 5)[blockIdx.x] = bmax;
    }
}

// KA: p <- r + beta (p - omega v);  v <- A K^-1 p;  partial rh.v
__global__ void k_kry_a(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ A_, int ashared,
                        KryVecs kv, int it, double rel_tol) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    KrylovCtl* ctl = kv.ctl + bz;
    if (ctl->done) return;
    double* part = kv.part + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    const int G = gridDim.x;
    double bnorm = (it == 0) ? reduce_partials(KP(part, 5), G, OpMax(), 0.0, smem) : ctl->bnorm;
    double rmax = reduce_partials(KP(part, 4), G, OpMax(), 0.0, smem);
    double rho_new = reduce_partials(KP(part, 0), G, OpSum(), 0.0, smem);
    if (rmax <= rel_tol * bnorm) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ctl->done = 1; ctl->iters = it; ctl->resid = bnorm != 0.0 ? rmax / bnorm : 0.0; ctl->bnorm = bnorm;
        }
        return;
    }
    const double rho_old = ctl->rho2[(it + 1) & 1], alpha = ctl->alpha, omega = ctl->omega;   // written by earlier kernels
    const double beta = (rho_new / rho_old) * (alpha / omega);
    const int64_t voff = (int64_t)bz * n;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    const double* r = kv.r + voff;
    const double* rh = kv.rh + voff;
    const double* pin = ((it & 1) ? kv.p1 : kv.p0) + voff;
    const double* vin = ((it & 1) ? kv.v1 : kv.v0) + voff;
    double* pout = ((it & 1) ? kv.p0 : kv.p1) + voff;
    double* vout = ((it & 1) ? kv.v0 : kv.v1) + voff;
    RowRange rr = block_rows(n);
    double rhv = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double pi = r[i] + beta * (pin[i] - omega * vin[i]);
        double acc = pi;   // A_ii * (p_i / A_ii)
        for (int s = 1; s < W; ++s) {
            int64_t idx = (int64_t)s * n + i;
            int j = cols[idx];
            double pj = r[j] + beta * (pin[j] - omega * vin[j]);
            acc += A[idx] * (pj / A[j]);
        }
        pout[i] = pi;
        vout[i] = acc;
        rhv += rh[i] * acc;
    }
    rhv = block_reduce(rhv, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) KP(part, 1)[blockIdx.x] = rhv;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->rho2[it & 1] = rho_new; if (it == 0) ctl->bnorm = bnorm; }
}

// KB: alpha = rho / rh.v;  s = r - alpha v;  t = A K^-1 s;  partials t.s, t.t
__global__ void k_kry_b(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ A_, int ashared,
                        KryVecs kv, int it) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    KrylovCtl* ctl = kv.ctl + bz;
    if (ctl->done) return;
    double* part = kv.part + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    const int G = gridDim.x;
    const double rhv = reduce_partials(KP(part, 1), G, OpSum(), 0.0, smem);
    const double alpha = ctl->rho2[it & 1] / rhv;
    const int64_t voff = (int64_t)bz * n;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    const double* r = kv.r + voff;
    const double* v = ((it & 1) ? kv.v0 : kv.v1) + voff;   // written by KA(it)
    double* sv = kv.s + voff;
    double* tv = kv.t + voff;
    RowRange rr = block_rows(n);
    double ts = 0.0, tt = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double si = r[i] - alpha * v[i];
        double acc = si;
        for (int s = 1; s < W; ++s) {
            int64_t idx = (int64_t)s * n + i;
            int j = cols[idx];
            acc += A[idx] * ((r[j] - alpha * v[j]) / A[j]);
        }
        sv[i] = si;
        tv[i] = acc;
        ts += acc * si;
        tt += acc * acc;
    }
    ts = block_reduce(ts, OpSum(), 0.0, smem);
    tt = block_reduce(tt, OpSum(), 0.0, smem);
    if (threadIdx.x == 0) { KP(part, 2)[blockIdx.x] = ts; KP(part, 3)[blockIdx.x] = tt; }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->alpha = alpha;
}

// KC: omega = t.s / t.t;  x += alpha K^-1 p + omega K^-1 s;  r = s - omega t;  partials rh.r, |r|max
__global__ void k_kry_c(int n, int W, const double* __restrict__ A_, int ashared, KryVecs kv, int it) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    KrylovCtl* ctl = kv.ctl + bz;
    if (ctl->done) return;
    double* part = kv.part + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    const int G = gridDim.x;
    const double ts = reduce_partials(KP(part, 2), G, OpSum(), 0.0, smem);
    const double tt = reduce_partials(KP(part, 3), G, OpSum(), 0.0, smem);
    const double omega = tt > 0.0 ? ts / tt : 0.0;
    const double alpha = ctl->alpha;
    const int64_t voff = (int64_t)bz * n;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    const double* p = ((it & 1) ? kv.p0 : kv.p1) + voff;   // written by KA(it)
    const double* sv = kv.s + voff;
    const double* tv = kv.t + voff;
    const double* rh = kv.rh + voff;
    double* x = kv.x + voff;
    double* r = kv.r + voff;
    RowRange rr = block_rows(n);
    double rho = 0.0, rmax = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double d = A[i];
        double si = sv[i];
        x[i] += alpha * (p[i] / d) + omega * (si / d);
        double ri = si - omega * tv[i];
        r[i] = ri;
        rho += rh[i] * ri;
        rmax = nan_max(rmax, fabs(ri));
    }
    rho = block_reduce(rho, OpSum(), 0.0, smem);
    rmax = block_reduce(rmax, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) { KP(part, 0)[blockIdx.x] = rho; KP(part, 4)[blockIdx.x] = rmax; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->omega = omega; ctl->iters = it + 1; }
}

// final bookkeeping + copy of the solution to its destination
__global__ void k_kry_finish(int n, KryVecs kv, VecRef out_ref, int64_t out_bs, int budget, double rel_tol) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    KrylovCtl* ctl = kv.ctl + bz;
    double* part = kv.part + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    if (!ctl->done) {
        double rmax = reduce_partials(KP(part, 4), gridDim.x, OpMax(), 0.0, smem);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            double bn = ctl->bnorm;
            ctl->resid = bn != 0.0 ? rmax / bn : 0.0;
            if (!(rmax <= rel_tol * bn)) ctl->flags |= FEMFCT_FLAG_SOLVER_BUDGET;
        }
    }
    const double* x = kv.x + (int64_t)bz * n;
    double* out = const_cast<double*>(vec_ptr(out_ref)) + bz * out_bs;
    RowRange rr = block_rows(n);
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) out[i] = x[i];
}

}  // namespace

namespace {
// Low-order solve by BiCGStab: publish its outcome in the step's control block (what the Jacobi
// sweeps / finalize_solve do otherwise) and evaluate the row-sum diagnostic from k_build_low's partials.
__global__ void k_kry_to_stepctl(const KrylovCtl* __restrict__ kc, StepCtl* __restrict__ sc, const double* __restrict__ part,
                                 int g_build) {
    __shared__ double smem[32];
    const int bz = blockIdx.x;
    const double* p = part + (int64_t)bz * 4 * FEMFCT_MAX_PARTIALS;
    double bnorm = reduce_partials(p + 2 * FEMFCT_MAX_PARTIALS, g_build, OpMax(), 0.0, smem);
    double rsmin = reduce_partials(p + 3 * FEMFCT_MAX_PARTIALS, g_build, OpMin(), INFINITY, smem);
    if (threadIdx.x == 0) {
        StepCtl* c = sc + bz;
        c->bnorm = bnorm;
        c->min_rowsum = rsmin;
        c->iters = kc[bz].iters;
        c->resid = kc[bz].resid;
        c->done = 1;
        c->parity = 0;
        int f = c->flags;
        if (!(rsmin > 0.0)) f |= FEMFCT_FLAG_MMATRIX_ROWSUM;
        if ((kc[bz].flags & FEMFCT_FLAG_SOLVER_BUDGET) || !(kc[bz].resid == kc[bz].resid)) f |= FEMFCT_FLAG_SOLVER_BUDGET;
        c->flags = f;
    }
}
}  // namespace

int femfct_enqueue_kry_to_stepctl(femfct_ctx* ctx, int g_build, int32_t batch) {
    hipLaunchKernelGGL(k_kry_to_stepctl, dim3(batch), dim3(256), 0, ctx->stream, (const KrylovCtl*)ctx->d_kry_ctl2, ctx->d_ctl,
                       ctx->d_part, g_build);
    return FEMFCT_OK;
}

int femfct_ensure_krylov_ws(femfct_ctx* ctx, int32_t batch) {
    const int om_cap = ctx->kry_max_iters + 16;
    if (batch <= ctx->kry_batch && om_cap <= ctx->chs_om_cap) return FEMFCT_OK;
    if (batch < ctx->kry_batch) batch = ctx->kry_batch;
    femfct_drop_graphs(ctx);
    if (ctx->d_chs_om) hipFree(ctx->d_chs_om);
    if (ctx->d_chs_scale) hipFree(ctx->d_chs_scale);
    ctx->d_chs_om = nullptr; ctx->d_chs_scale = nullptr; ctx->chs_om_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_chs_om, sizeof(double) * (size_t)batch * om_cap));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_chs_scale, sizeof(double) * (size_t)batch));
    ctx->chs_om_cap = om_cap;
    if (ctx->d_kry) hipFree(ctx->d_kry);
    if (ctx->d_kry_part) hipFree(ctx->d_kry_part);
    if (ctx->d_kry_ctl) hipFree(ctx->d_kry_ctl);
    ctx->d_kry = nullptr; ctx->d_kry_part = nullptr; ctx->d_kry_ctl = nullptr; ctx->kry_batch = 0;
    size_t nv = (size_t)batch * ctx->n;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_kry, sizeof(double) * nv * 9));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_kry_part, sizeof(double) * (size_t)batch * 6 * FEMFCT_MAX_PARTIALS));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_kry_ctl, sizeof(KrylovCtl) * (size_t)batch));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_kry_ctl, 0, sizeof(KrylovCtl) * batch, ctx->stream));
    if (ctx->d_kry_ctl2) hipFree(ctx->d_kry_ctl2);
    ctx->d_kry_ctl2 = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_kry_ctl2, sizeof(KrylovCtl) * (size_t)batch));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_kry_ctl2, 0, sizeof(KrylovCtl) * batch, ctx->stream));
    ctx->kry_batch = batch;
    return FEMFCT_OK;
}

int femfct_enqueue_bicgstab(femfct_ctx* ctx, const double* mat, int32_t mat_shared, const double* b, VecRef x0,
                            int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget, bool lowsolve) {
    const size_t nv = (size_t)ctx->kry_batch * ctx->n;
    KryVecs kv;
    double* base = ctx->d_kry;
    kv.x = base; kv.r = base + nv; kv.rh = base + 2 * nv; kv.p0 = base + 3 * nv; kv.p1 = base + 4 * nv;
    kv.v0 = base + 5 * nv; kv.v1 = base + 6 * nv; kv.s = base + 7 * nv; kv.t = base + 8 * nv;
    kv.part = ctx->d_kry_part;
    kv.ctl = (KrylovCtl*)(lowsolve ? ctx->d_kry_ctl2 : ctx->d_kry_ctl);
    const double tol = lowsolve ? ctx->rel_tol : ctx->kry_tol;
    LaunchGeom g = femfct_geom(ctx, batch);
    hipStream_t st = ctx->stream;
    const int n = ctx->n, W = ctx->W;
    femfct_prof_begin(ctx, KC_OTHER);
    hipLaunchKernelGGL(k_kry_init, g.grid, g.block, 0, st, n, W, ctx->d_cols, mat, mat_shared, b, x0, x0_bs, kv);
    for (int it = 0; it < budget; ++it) {
        hipLaunchKernelGGL(k_kry_a, g.grid, g.block, 0, st, n, W, ctx->d_cols, mat, mat_shared, kv, it, tol);
        hipLaunchKernelGGL(k_kry_b, g.grid, g.block, 0, st, n, W, ctx->d_cols, mat, mat_shared, kv, it);
        hipLaunchKernelGGL(k_kry_c, g.grid, g.block, 0, st, n, W, mat, mat_shared, kv, it);
    }
    // one more convergence test of the last residual happens in k_kry_finish
    hipLaunchKernelGGL(k_kry_finish, g.grid, g.block, 0, st, n, kv, x_out, out_bs, budget, tol);
    femfct_prof_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return femfct_fail(ctx, FEMFCT_ERR_HIP, "bicgstab launch failed: %s", hipGetErrorString(e));
    return FEMFCT_OK;
}


// ===========================================================================================
// Chebyshev species solve: the same implicit systems as the BiCGStab above, for the structured
// 7-point mesh in vertex order.  Dot-product free, so ten iterations run inside one tile launch
// (k_tile_cheb / k_tile4_cheb with the system matrix instead of M): ~10x fewer launches per solve.
//   spectrum of D^-1 Mat:  lambda_max <= 2 x (1 + safety) on the right-diagonal P1 mesh (element
//   matrices of M, Ad and the weighted masses all satisfy Me <= 2 diag(Me)); lambda_min >= 0.5 min_i
//   m_ii / a_ii because sym(Mat) >= M >= 0.5 diag(M).  The skew (convective) part only bends the
//   spectrum into an ellipse around that interval; the residual check below decides, and the sweep
//   falls back to BiCGStab when the iteration does not contract.
// ===========================================================================================
namespace {

// one block per batch member: lambda_min bound, omega table (closed form of the three-term
// recurrence w_1 = 1, w_{k+1} = 2 xi T_k(xi) / T_{k+1}(xi), xi = 1/rho).
//   tau >= 0: Mat = M + tau*Ad + (terms with positive semi-definite symmetric part); then
//     lambda_min >= lam_e * min_i (m_ii + tau k_ii) / a_ii,   lam_e = smallest eigenvalue of the element
//     pencil (Me + tau Ke, diag(Me + tau Ke)) (element-by-element bound, host-computed);
//   tau < 0 (structure unknown): lambda_min >= 0.5 min_i m_ii / a_ii.
__global__ void k_chs_setup(int n, int W, const double* __restrict__ A_, int ashared, const double* __restrict__ Mdiag,
                            const double* __restrict__ Kdiag, double tau, double lam_e, double lmax, int K,
                            double* __restrict__ om, int om_bs, double* __restrict__ scale, KrylovCtl* __restrict__ ctl_) {
    __shared__ double smem[32];
    const int bz = blockIdx.x;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    double mn = INFINITY;
    if (tau >= 0.0)
        for (int i = threadIdx.x; i < n; i += blockDim.x) mn = fmin(mn, (Mdiag[i] + tau * Kdiag[i]) / A[i]);
    else
        for (int i = threadIdx.x; i < n; i += blockDim.x) mn = fmin(mn, Mdiag[i] / A[i]);
    mn = block_reduce(mn, OpMin(), INFINITY, smem);
    double lmin = 0.9 * lam_e * fmin(mn, 1.0);
    if (!(lmin > 0.0) || !(lmin < lmax)) lmin = 0.5 * lmax;   // not an M + dt*(...) system: the check will tell
    const double rho = (lmax - lmin) / (lmax + lmin);
    const double xi = 1.0 / rho;
    const double theta = log(xi + sqrt(xi * xi - 1.0));
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        double w = 1.0;
        if (k > 0) w = 2.0 * xi * exp(-theta) * (1.0 + exp(-2.0 * k * theta)) / (1.0 + exp(-2.0 * (k + 1) * theta));
        om[(int64_t)bz * om_bs + k] = w;
    }
    if (threadIdx.x == 0) {
        scale[bz] = 0.5 * (lmin + lmax);
        KrylovCtl* c = ctl_ + bz;
        c->flags = 0; c->iters = 0; c->done = 0; c->resid = 0.0; c->bnorm = 0.0;
        c->alpha = theta;   // asymptotic contraction exp(-theta) per iteration
        c->omega = lmin;
    }
}

// r = b - A x: per-block max |r|, max |b|, max (|A| |x|)_i (the rounding scale of the residual, see k_chs_finish)
__global__ void k_chs_check(int n, int W, const int32_t* __restrict__ cols, const double* __restrict__ A_, int ashared,
                            const double* __restrict__ b_, VecRef x_ref, int64_t x_bs, double* __restrict__ part_) {
    __shared__ double smem[32];
    const int bz = blockIdx.y;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * W * n);
    const double* b = b_ + (int64_t)bz * n;
    const double* x = vec_ptr(x_ref) + bz * x_bs;
    double* part = part_ + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    RowRange rr = block_rows(n);
    double rmax = 0.0, bmax = 0.0, amax = 0.0;
    for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
        double acc = A[i] * x[i];
        double aabs = fabs(acc);
        for (int s = 1; s < W; ++s) {
            int64_t idx = (int64_t)s * n + i;
            const double t = A[idx] * x[cols[idx]];
            acc += t;
            aabs += fabs(t);
        }
        const double bi = b[i];
        const double ri = fabs(bi - acc);
        rmax = (ri == ri) ? fmax(rmax, ri) : INFINITY;
        bmax = nan_max(bmax, fabs(bi));
        amax = nan_max(amax, aabs);
    }
    rmax = block_reduce(rmax, OpMax(), 0.0, smem);
    bmax = block_reduce(bmax, OpMax(), 0.0, smem);
    amax = block_reduce(amax, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) { KP(part, 3)[blockIdx.x] = amax; KP(part, 4)[blockIdx.x] = rmax; KP(part, 5)[blockIdx.x] = bmax; }
}

// The true residual b - A x of a computed x cannot fall below the rounding of A x itself, ~eps max_i (|A| |x|)_i.  For a
// species matrix M + dt (D Ad + ...) with dt D / h^2 >> 1 that is ~eps dt D / h^2 ||b||: already 3e-14 ||b|| for the
// Schnakenberg solve on 81^2 nodes (dt = 5e-4), 5e-13 ||b|| on 301^2 -- a test against rel_tol = 1e-13 alone would never
// pass there.  The Chebyshev check therefore measures the residual against the larger of ||b|| and CHS_FLOOR ulps of
// |A| |x| over rel_tol: below CHS_FLOOR eps max (|A| |x|) the residual is rounding noise (a backward error of CHS_FLOOR
// eps), where rel_tol ||b|| is reachable the test is the plain relative one.
#define CHS_FLOOR 32.0

// iters reports the iteration count that would have met tol/10 at the asymptotic rate (the host
// sizes the next sweep's budget from it); FEMFCT_FLAG_SOLVER_BUDGET when this solve missed tol.  resid is relative to
// the larger of ||b|| and the rounding scale above.
__global__ void k_chs_finish(const double* __restrict__ part_, int G, KrylovCtl* __restrict__ ctl_, int K, double rel_tol) {
    __shared__ double smem[32];
    const int bz = blockIdx.x;
    const double* part = part_ + (int64_t)bz * 6 * FEMFCT_MAX_PARTIALS;
    const double rmax = reduce_partials(KP(part, 4), G, OpMax(), 0.0, smem);
    const double bmax = reduce_partials(KP(part, 5), G, OpMax(), 0.0, smem);
    const double amax = reduce_partials(KP(part, 3), G, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) {
        KrylovCtl* c = ctl_ + bz;
        const double scale = rel_tol > 0.0 ? nan_max(bmax, CHS_FLOOR * DBL_EPSILON * amax / rel_tol) : bmax;
        const double res = scale != 0.0 ? rmax / scale : (rmax == 0.0 ? 0.0 : INFINITY);
        c->resid = res;
        c->bnorm = bmax;
        c->done = 1;
        const double theta = c->alpha;
        double need = K;
        if (res > 0.0 && res < INFINITY) need = K + log(res / (0.1 * rel_tol)) / theta;
        else if (res == 0.0) need = 1.0;
        need = fmin(fmax(need, 1.0), 1.0e6);
        c->iters = (int)ceil(need);
        c->flags |= FEMFCT_FLAG_CHEBYSHEV;
        if (!(res <= rel_tol)) c->flags |= FEMFCT_FLAG_SOLVER_BUDGET;
    }
}

}  // namespace

// smallest eigenvalue of diag(Ae)^-1 Ae, Ae = Me + tau*Ke of the right-angled P1 element with legs h
// (both triangle orientations are congruent): symmetric 3x3, trigonometric formula
static double element_lambda_min(double h, double tau) {
    const double T = 0.5 * h * h;
    const double Me[3][3] = {{T / 6, T / 12, T / 12}, {T / 12, T / 6, T / 12}, {T / 12, T / 12, T / 6}};
    const double Ke[3][3] = {{1.0, -0.5, -0.5}, {-0.5, 0.5, 0.0}, {-0.5, 0.0, 0.5}};
    double S[3][3], d[3];
    for (int i = 0; i < 3; ++i) d[i] = 1.0 / sqrt(Me[i][i] + tau * Ke[i][i]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i][j] = d[i] * (Me[i][j] + tau * Ke[i][j]) * d[j];
    const double p1 = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
    const double q = (S[0][0] + S[1][1] + S[2][2]) / 3.0;
    const double p2 = (S[0][0] - q) * (S[0][0] - q) + (S[1][1] - q) * (S[1][1] - q) + (S[2][2] - q) * (S[2][2] - q) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    if (!(p > 0.0)) return q;
    double B[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) B[i][j] = (S[i][j] - (i == j ? q : 0.0)) / p;
    double r = 0.5 * (B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0]) +
                      B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]));
    r = std::min(1.0, std::max(-1.0, r));
    const double phi = acos(r) / 3.0;
    return q + 2.0 * p * cos(phi + 2.0 * M_PI / 3.0);
}

bool femfct_species_cheb(const femfct_ctx* ctx, int kind) {
    const auto st = ctx->kinds.find(kind);
    if (ctx->species_solver != 0 || (st != ctx->kinds.end() && st->second.cheb_off)) return false;
    if (ctx->structured && femfct_mesh_solve_fits(ctx)) return true;     // one workgroup per system (any ordering)
    if (!femfct_tiles_usable(ctx)) return false;
    TilePlan tp;
    return femfct_tile_plan(ctx, &tp, false);
}

// iterations per launch of the species solve: the tile plan of an iteration budget (deep halos while
// every workgroup gets its own CU: 214 iterations = 17 launches of 13 instead of 22 of 10)
static bool species_plan(const femfct_ctx* ctx, TilePlan* tp, int32_t batch, int32_t budget) {
    return femfct_tile_plan(ctx, tp, false, budget > 0 ? budget : 0, batch);
}

// -------------------------------------------------------------------------------------------
// The whole species solve in ONE launch for meshes that fit a workgroup (n <= 1024 * NPT): one workgroup per
// batch member keeps the iterate in LDS (three rotating buffers indexed by node), the rows pre-scaled in
// registers, and runs the spectrum bound (k_chs_setup), every Chebyshev iteration, the convergence test and the
// bookkeeping (k_chs_check / k_chs_finish) itself -- __syncthreads() is the only synchronisation.  The omegas come
// from the three-term recurrence; z = rmd * r is the scaled residual of the current iterate, so the workgroup
// tests ||r||_inf <= tol ||b||_inf every CHECK iterations and stops by itself (iters = the exact count).
// Any ELL pattern / ordering (neighbours through the column table).  Configs C3/C4 (n = 1681): 221 iterations of
// the Schnakenberg solve take one launch instead of 17 tile launches + 3 bookkeeping launches.
// -------------------------------------------------------------------------------------------
namespace {

template <int NPT>
__global__ void __launch_bounds__(1024)
k_mesh_cheb_solve(int n, int Wrt, const int32_t* __restrict__ cols, const double* __restrict__ A_, int ashared,
                  const double* __restrict__ b_, VecRef x0_ref, int64_t x0_bs, VecRef out_ref, int64_t out_bs,
                  const double* __restrict__ Mdiag, const double* __restrict__ Kdiag, double tau, double lam_e, double lmax,
                  int K, double rel_tol, KrylovCtl* __restrict__ ctl_, EndArgs e) {
    constexpr int CHECK = 16, W = 7;      // structured P1 mesh: seven slots (checked by the launcher)
    // e.level != null: this solve is the last operation of its time step -- every workgroup logs its own records and the
    // last one of the graph's last step moves the time level (as k_mesh_step does); the ordinal is read before anything else
    const int ord = e.level ? e.level[1] + e.ord_off : 0;
    extern __shared__ double ybuf[];          // 2 * n doubles: the iterate the neighbours read, and the next one
    __shared__ double smem[32];
    const int bz = blockIdx.x;
    const double* A = A_ + (ashared ? 0 : (int64_t)bz * Wrt * n);
    const double* b = b_ + (int64_t)bz * n;
    const double* x0 = vec_ptr(x0_ref) + bz * x0_bs;
    double* out = const_cast<double*>(vec_ptr(out_ref)) + bz * out_bs;
    double* const B0 = ybuf;
    double* const B1 = ybuf + n;
    // spectrum bound of D^-1 A (see k_chs_setup)
    double mn = INFINITY, bmax = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        mn = fmin(mn, (tau >= 0.0 ? Mdiag[i] + tau * Kdiag[i] : Mdiag[i]) / A[i]);
        bmax = nan_max(bmax, fabs(b[i]));
    }
    mn = block_reduce(mn, OpMin(), INFINITY, smem);
    bmax = block_reduce(bmax, OpMax(), 0.0, smem);
    double lmin = 0.9 * lam_e * fmin(mn, 1.0);
    if (!(lmin > 0.0) || !(lmin < lmax)) lmin = 0.5 * lmax;
    const double rho = (lmax - lmin) / (lmax + lmin);
    const double scale = 0.5 * (lmin + lmax), inv_scale = 1.0 / scale;
    const double xi = 1.0 / rho, theta = log(xi + sqrt(xi * xi - 1.0));
    // rows of the thread's nodes, scaled by 1 / (scale * a_ii)
    int idx[NPT], nb[NPT][W - 1];
    double ms[NPT][W - 1], bs[NPT], sa[NPT], ym[NPT], yo[NPT];
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const int i = threadIdx.x + q * 1024;
        idx[q] = i < n ? i : -1;
        bs[q] = 0.0; sa[q] = 1.0; ym[q] = 0.0; yo[q] = 0.0;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) { ms[q][s] = 0.0; nb[q][s] = 0; }
        if (i < n) {
            sa[q] = scale * A[i];
            const double rmd = 1.0 / sa[q];
#pragma unroll
            for (int s = 1; s < W; ++s) {
                const int64_t e = (int64_t)s * n + i;
                ms[q][s - 1] = A[e] * rmd;
                nb[q][s - 1] = cols[e];
            }
            bs[q] = b[i] * rmd;
            ym[q] = x0[i];
            B0[i] = ym[q];
        }
    }
    __syncthreads();
    double omega = 1.0, res = INFINITY;
    int k = 0;
#pragma unroll 2
    for (; k < K; ++k) {
        // y_{k-1} lives in registers only; the two LDS buffers alternate by the parity of k (unrolled by two, so
        // every LDS access has a constant base)
        const double* y_mid = (k & 1) ? B1 : B0;
        double* y_new = (k & 1) ? B0 : B1;
        double zmax = 0.0;
        double yn[NPT];
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            double z = fma(-inv_scale, ym[q], bs[q]);
#pragma unroll
            for (int s = 0; s < W - 1; ++s) z = fma(-ms[q][s], y_mid[nb[q][s]], z);
            zmax = nan_max(zmax, fabs(z) * sa[q]);                 // |r_i| of the current iterate
            yn[q] = omega * (z + ym[q] - yo[q]) + yo[q];
        }
        if ((k % CHECK) == 0) {                                  // uniform decision: everybody reduces the same value
            res = block_reduce(zmax, OpMax(), 0.0, smem);
            if (res <= rel_tol * bmax) break;                    // the current iterate already meets the tolerance
        }
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            if (idx[q] >= 0) y_new[idx[q]] = yn[q];
            yo[q] = ym[q];
            ym[q] = yn[q];
        }
        __syncthreads();
        omega = (k == 0) ? 1.0 / (1.0 - 0.5 * rho * rho) : 1.0 / (1.0 - 0.25 * rho * rho * omega);
    }
    if (k == K) {                                                // budget exhausted: residual of the last iterate
        const double* y_mid = (k & 1) ? B1 : B0;
        double zmax = 0.0;
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            double z = fma(-inv_scale, ym[q], bs[q]);
#pragma unroll
            for (int s = 0; s < W - 1; ++s) z = fma(-ms[q][s], y_mid[nb[q][s]], z);
            zmax = nan_max(zmax, fabs(z) * sa[q]);
        }
        res = block_reduce(zmax, OpMax(), 0.0, smem);
    }
#pragma unroll
    for (int q = 0; q < NPT; ++q)
        if (idx[q] >= 0) out[idx[q]] = ym[q];
    if (threadIdx.x == 0) {
        KrylovCtl* c = ctl_ + bz;
        const double rr = bmax != 0.0 ? res / bmax : (res == 0.0 ? 0.0 : INFINITY);
        c->flags = FEMFCT_FLAG_CHEBYSHEV;
        c->done = 1;
        c->resid = rr;
        c->bnorm = bmax;
        c->alpha = theta;
        c->omega = lmin;
        if (rr <= rel_tol) {
            c->iters = k + CHECK;      // the test runs every CHECK iterations: an upper bound of what was needed
        } else {
            double need = K;
            if (rr < INFINITY) need = K + log(rr / (0.1 * rel_tol)) / theta;
            c->iters = (int)ceil(fmin(fmax(need, 1.0), 1.0e6));
            c->flags |= FEMFCT_FLAG_SOLVER_BUDGET;
        }
        if (e.level) e.klog[(int64_t)ord * e.batch + bz] = *c;
    }
    if (e.level) {
        const uint32_t* cs = reinterpret_cast<const uint32_t*>(e.ctl + bz);        // the FCT step's record (an earlier kernel's)
        uint32_t* cd = reinterpret_cast<uint32_t*>(e.log + (int64_t)ord * e.batch + bz);
        if (threadIdx.x >= 64 && threadIdx.x < 80) cd[threadIdx.x - 64] = cs[threadIdx.x - 64];
        if (e.ord_adv != 0) {
            __syncthreads();
            if (threadIdx.x == 0) {
                __threadfence();
                if (atomicAdd(e.ticket, 1u) == gridDim.x - 1) {
                    e.level[0] += e.delta;
                    e.level[1] = (ord - e.ord_off) + e.ord_adv;
                    *e.ticket = 0u;
                }
            }
        }
    }
}

}  // namespace

// meshes whose species solve runs as one workgroup per system
// (two nodes per thread; the four-node variant for n <= 4096 spills at 128 VGPRs and is not used)
bool femfct_mesh_solve_fits(const femfct_ctx* ctx) { return ctx->mesh_solve && ctx->n <= 2048 && ctx->W == 7; }

static int enqueue_mesh_cheb_solve(femfct_ctx* ctx, const double* mat, int32_t mat_shared, const double* b, VecRef x0,
                                   int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget, double tau) {
    const int n = ctx->n, W = ctx->W;
    const double lam_e = tau >= 0.0 ? element_lambda_min(ctx->h, tau) : 0.5;
    const size_t lds = (size_t)2 * n * sizeof(double);
    KrylovCtl* ctl = (KrylovCtl*)ctx->d_kry_ctl;
    // last operation of a time step (femfct_request_fused_end): the kernel logs and advances itself, no k_step_end launch
    EndArgs e{};
    const bool fuse_end = ctx->end_req_delta != 0 && ctx->end_req_krylov && ctx->d_ticket && ctx->d_level && ctx->d_log &&
                          ctx->d_klog && !ctx->prof_on;
    if (fuse_end) {
        e.level = ctx->d_level; e.delta = ctx->rep_last ? ctx->end_req_delta * ctx->rep_total : 0;
        e.ord_adv = ctx->rep_last ? ctx->rep_total : 0; e.ord_off = ctx->ord_bias; e.ctl = ctx->d_ctl; e.log = ctx->d_log;
        e.kctl = ctl; e.klog = (KrylovCtl*)ctx->d_klog; e.batch = batch; e.ticket = ctx->d_ticket;
    }
    femfct_prof_begin(ctx, KC_OTHER);
#define MS(NPT)                                                                                                          \
    do {                                                                                                                 \
        if (!ctx->mesh_solve_attr[NPT])                                                                                  \
            HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_mesh_cheb_solve<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                             2 * 1024 * NPT * 8));                                                       \
        ctx->mesh_solve_attr[NPT] = true;                                                                                \
        hipLaunchKernelGGL((k_mesh_cheb_solve<NPT>), dim3(batch), dim3(1024), lds, ctx->stream, n, W, ctx->d_cols, mat,  \
                           mat_shared, b, x0, x0_bs, x_out, out_bs, (const double*)ctx->d_M, (const double*)ctx->d_Ad, tau, \
                           lam_e, 2.2, (int)budget, ctx->kry_tol, ctl, e);                                               \
    } while (0)
    MS(2);
#undef MS
    femfct_prof_end(ctx);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return femfct_fail(ctx, FEMFCT_ERR_HIP, "Chebyshev solve launch failed: %s", hipGetErrorString(err));
    if (fuse_end) ctx->end_fused = true;
    return FEMFCT_OK;
}

int femfct_cheb_depth(const femfct_ctx* ctx, int32_t batch, int32_t budget) {
    if (femfct_single_patch(ctx, batch)) return std::max(1, (int)budget);   // all iterations in one launch
    if (femfct_tile4_wanted(ctx, batch)) return 10;
    TilePlan tp;
    species_plan(ctx, &tp, batch, budget);
    return tp.K;
}

int femfct_enqueue_cheb_solve(femfct_ctx* ctx, const double* mat, int32_t mat_shared, const double* b, VecRef x0,
                              int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget, double tau) {
    if (femfct_mesh_solve_fits(ctx))
        return enqueue_mesh_cheb_solve(ctx, mat, mat_shared, b, x0, x0_bs, x_out, out_bs, batch, budget, tau);
    const int n = ctx->n, W = ctx->W;
    const int depth = femfct_cheb_depth(ctx, batch, budget);
    int K = ((budget + depth - 1) / depth) * depth;
    if (K > ctx->chs_om_cap) K = (ctx->chs_om_cap / depth) * depth;
    KrylovCtl* ctl = (KrylovCtl*)ctx->d_kry_ctl;
    hipStream_t st = ctx->stream;
    femfct_prof_begin(ctx, KC_OTHER);
    const double lam_e = tau >= 0.0 ? element_lambda_min(ctx->h, tau) : 0.5;
    hipLaunchKernelGGL(k_chs_setup, dim3(batch), dim3(1024), 0, st, n, W, mat, mat_shared, (const double*)ctx->d_M,
                       (const double*)ctx->d_Ad, tau, lam_e, 2.2, K, ctx->d_chs_om, ctx->chs_om_cap, ctx->d_chs_scale, ctl);
    femfct_prof_end(ctx);
    ChebIO io{};
    io.mat = mat; io.mat_bs = mat_shared ? 0 : (int64_t)W * n;
    io.mid_ref = x0; io.mid_bs = x0_bs;
    io.out_ref = x_out; io.out_bs = out_bs;
    io.om_dev = ctx->d_chs_om; io.om_bs = ctx->chs_om_cap; io.scale_dev = ctx->d_chs_scale;
    int rc;
    // y_out pointer is a placeholder: the last launch writes through io.out_ref
    if (femfct_tile4_wanted(ctx, batch) || femfct_single_patch(ctx, batch)) {
        rc = femfct_enqueue_tile4_cheb(ctx, b, nullptr, nullptr, ctx->d_y0, 1, K, nullptr, 1.0, ctx->d_y0, ctx->d_y2, ctx->d_y1,
                                       ctx->d_rp, batch, &io);
    } else {
        TilePlan tp;
        species_plan(ctx, &tp, batch, budget);
        rc = femfct_enqueue_tile_cheb(ctx, tp, b, nullptr, nullptr, ctx->d_y0, 1, K, nullptr, 1.0, ctx->d_y0, ctx->d_y2,
                                      ctx->d_y1, ctx->d_rp, batch, &io);
    }
    if (rc != FEMFCT_OK) return rc;
    LaunchGeom g = femfct_geom(ctx, batch);
    femfct_prof_begin(ctx, KC_OTHER);
    hipLaunchKernelGGL(k_chs_check, g.grid, g.block, 0, st, n, W, ctx->d_cols, mat, mat_shared, b, x_out, out_bs, ctx->d_kry_part);
    hipLaunchKernelGGL(k_chs_finish, dim3(batch), dim3(256), 0, st, (const double*)ctx->d_kry_part, (int)g.grid.x, ctl, K,
                       ctx->kry_tol);
    femfct_prof_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return femfct_fail(ctx, FEMFCT_ERR_HIP, "Chebyshev solve launch failed: %s", hipGetErrorString(e));
    return FEMFCT_OK;
}

// the species solve of a trajectory sweep of the given kind
int femfct_enqueue_species_solve(femfct_ctx* ctx, int kind, const double* mat, int32_t mat_shared, const double* b,
                                 VecRef x0, int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget,
                                 double tau) {
    if (femfct_species_cheb(ctx, kind))
        return femfct_enqueue_cheb_solve(ctx, mat, mat_shared, b, x0, x0_bs, x_out, out_bs, batch, budget, tau);
    return femfct_enqueue_bicgstab(ctx, mat, mat_shared, b, x0, x0_bs, x_out, out_bs, batch, budget);
}
