// Device primitive of the control budget ||c||_{1,h} <= B in the proximal-gradient loops (solvers.prox_solidbody,
// solvers.prox_source_control with budget=; an extension, no reference call):
//   femfct_budget_trials   the K Armijo trials c_t = clip(soft_threshold(c + s_t d, s_t alpha + lambda_t)), lambda_t >= 0 the
//                          smallest value with ||c_t||_{1,h} <= B, their sources, multipliers and norms
// Only scalars cross PCIe: per search round 19 doubles per trial.
//
// phi_t(theta) = ||clip(soft_threshold(x_t, theta))||_{1,h} is continuous, piecewise linear and non-increasing in the total
// threshold theta.  The trials are first written with lambda = 0 (femfct_prox_trials' bits) together with their norms and
// max |x_t|; a trial over budget then has a bracket [a, b] = [tau_t, max |x_t|] with phi(a) > B >= phi(b) = 0.  A round
// is one launch over all such trials: phi at the 15 interior points of a 16-way split, and the three sums and the count
// that decide whether phi is affine on the bracket (no value changes between zero, linear and clipped inside it), in
// which case the root is closed form.  The host keeps the sub-interval where phi crosses B (femfct_budget_narrow).
// Trials over budget are written again with their lambda.
//
// Determinism: no atomics, fixed trees.  The writing kernel has k_l1_partials' row partition and block_reduce tree and is
// folded by k_reduce_levels, so its norm is femfct_l1_norm_Q of what it wrote, bit for bit.  The rounds only steer the
// search; they use fewer, larger blocks (19 sums per item would otherwise be mostly reduction).
#include "femfct_internal.h"
#include "device_utils.h"
#include "prox_device.h"
#include <math.h>

namespace {

// per-trial launch parameters (by value: K <= FEMFCT_MAX_TRIALS)
struct BudgetWrite { double lam[FEMFCT_MAX_TRIALS]; int32_t active[FEMFCT_MAX_TRIALS]; };
struct BudgetRound { double a[FEMFCT_MAX_TRIALS], b[FEMFCT_MAX_TRIALS]; int32_t active[FEMFCT_MAX_TRIALS]; };

// point j = 0 .. 16 of the split of [a, b]; non-decreasing in j, within [a, b]; host and device evaluate the same expression
__host__ __device__ __forceinline__ double budget_point(double a, double b, int j) { return a + (b - a) * (j * 0.0625); }

// For the items q = t*levels + l of the active trials (strided over gridDim.y) and this block's rows (k_l1_partials'
// partition): c_out[q*n + i] = prox_value(c, s_t, d, s_t alpha + lam_t), src_out = 1.0*g + 1.0*c_t (g NULL: c_t; src_out
// NULL: none), part_l[q*G + block] = k_l1_partials' partial of what was written, part_m[q*G + block] = max |c + s_t d|
// (a NaN carried).  d NULL: x = c (s_t = 0, K = 1).
__global__ void __launch_bounds__(256) k_budget_write(int n, const double* __restrict__ ml, const double* __restrict__ c,
                                                      const double* __restrict__ d, const double* __restrict__ g, double s0,
                                                      double alpha, double lo, double hi, int levels, int64_t items,
                                                      BudgetWrite par, double* __restrict__ c_out,
                                                      double* __restrict__ src_out, double* __restrict__ part_l,
                                                      double* __restrict__ part_m) {
    __shared__ double smem[64];
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int t = (int)(q / levels);
        if (!par.active[t]) continue;       // (uniform over the block)
        const int64_t lvl = q % levels;
        const double s = d ? s0 * (1.0 / (double)(1 << t)) : 0.0;
        const double tau = s * alpha;
        const double th = tau + par.lam[t];
        const double* cl = c + lvl * n;
        const double* dl = d ? d + lvl * n : nullptr;
        const double* gl = g ? g + lvl * n : nullptr;
        double* ol = c_out + q * n;
        double* sl = src_out ? src_out + q * n : nullptr;
        double sum = 0.0, mx = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double ci = cl[i], di = dl ? dl[i] : 0.0;
            const double v = prox_value(ci, s, di, th, lo, hi);
            ol[i] = v;
            if (sl) sl[i] = gl ? 1.0 * gl[i] + 1.0 * v : v;
            sum += ml[i] * fabs(v);
            mx = nan_max(mx, fabs(ci + s * di));
        }
        sum = block_reduce(sum, OpSum(), 0.0, smem);
        mx = block_reduce(mx, OpMax(), 0.0, smem + 32);
        if (threadIdx.x == 0) {
            part_l[q * gridDim.x + blockIdx.x] = sum;
            part_m[q * gridDim.x + blockIdx.x] = mx;
        }
    }
}

// out[t] = max of the per_trial partials of trial t (a NaN carried)
__global__ void __launch_bounds__(256) k_budget_max_fold(int64_t per_trial, const double* __restrict__ part,
                                                         double* __restrict__ out) {
    __shared__ double smem[32];
    const double* p = part + (int64_t)blockIdx.x * per_trial;
    double m = 0.0;
    for (int64_t k = threadIdx.x; k < per_trial; k += blockDim.x) m = nan_max(m, p[k]);
    m = block_reduce(m, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// One search round.  For the items q = t*levels + l of the active trials and this block's rows, with x = c + s_t d,
// w = ml_i, bound = hi (x > 0) or -lo (x < 0), z = |x| (the threshold from which the value is zero) and
// y = |x| - bound (the threshold up to which it sits at its bound), the sums over the rows of
//   j < 15     w * min(|x| - p_j, bound) where |x| > p_j       p_j = budget_point(a_t, b_t, j + 1): phi at the interior points
//   15 S_fix   w * bound   where y >= b                         (clipped on all of (a, b))
//   16 S_lin   w * |x|     where y <= a and z >= b              (linear on all of (a, b))
//   17 W       w           over the same values
//   cnt        1           where the value changes class inside (a, b); a zero bound never contributes and never counts
// part_s[((t*18 + j)*levels + l)*G + block], part_c[(t*levels + l)*G + block]: k_reduce_levels' layout, batch K*18 and K.
__global__ void __launch_bounds__(256) k_budget_round(int n, const double* __restrict__ ml, const double* __restrict__ c,
                                                      const double* __restrict__ d, double s0, double lo, double hi,
                                                      int levels, int64_t items, BudgetRound par,
                                                      double* __restrict__ part_s, double* __restrict__ part_c) {
    __shared__ double smem[32];
    const int G = gridDim.x;
    RowRange rr = block_rows(n);
    for (int64_t q = blockIdx.y; q < items; q += gridDim.y) {
        const int t = (int)(q / levels);
        if (!par.active[t]) continue;
        const int64_t lvl = q % levels;
        const double s = d ? s0 * (1.0 / (double)(1 << t)) : 0.0;
        const double a = par.a[t], b = par.b[t];
        const double* cl = c + lvl * n;
        const double* dl = d ? d + lvl * n : nullptr;
        double acc[BUDGET_SUMS];
#pragma unroll
        for (int j = 0; j < BUDGET_SUMS; ++j) acc[j] = 0.0;
        double cnt = 0.0;
        for (int i = rr.begin + threadIdx.x; i < rr.end; i += blockDim.x) {
            const double x = cl[i] + s * (dl ? dl[i] : 0.0);
            const double w = ml[i], z = fabs(x);
            const double bound = x > 0 ? hi : -lo;
            if (!(bound > 0.0)) continue;           // the value is 0 for every threshold
#pragma unroll
            for (int j = 0; j < BUDGET_POINTS; ++j) {
                const double r = z - budget_point(a, b, j + 1);
                if (r > 0) acc[j] += w * fmin(r, bound);
            }
            const double y = z - bound;
            if (z <= a) {
            } else if (y >= b) {
                acc[BUDGET_POINTS] += w * bound;
            } else if (y <= a && z >= b) {
                acc[BUDGET_POINTS + 1] += w * z;
                acc[BUDGET_POINTS + 2] += w;
            } else {
                cnt += 1.0;
            }
        }
#pragma unroll
        for (int j = 0; j < BUDGET_SUMS; ++j) {
            const double r = block_reduce(acc[j], OpSum(), 0.0, smem);
            if (threadIdx.x == 0) part_s[(((int64_t)t * BUDGET_SUMS + j) * levels + lvl) * G + blockIdx.x] = r;
        }
        cnt = block_reduce(cnt, OpSum(), 0.0, smem);      // integers below 2^53: exact in any order
        if (threadIdx.x == 0) part_c[q * G + blockIdx.x] = cnt;
    }
}

unsigned grid_y(int64_t work) { return (unsigned)(work < 65535 ? work : 65535); }

}  // namespace

// What a round's read-back v (BUDGET_VALS doubles: phi at the 15 interior points, S_fix, S_lin, W, count) means for one
// trial's bracket [*a, *b].  Returns true with the total threshold in *th when the search of this trial is over, false
// after narrowing the bracket to the sub-interval where phi crosses the budget.  Written for any values of v: a NaN, an
// infinity or a nonsensical count only ever ends the search at b, the feasible end, or narrows the bracket.
bool femfct_budget_narrow(double* a, double* b, const double* v, double budget, double* th) {
    const double a0 = *a, b0 = *b;
    if (!(b0 > a0)) { *th = b0; return true; }
    if (v[BUDGET_SUMS] == 0.0) {      // no value changes class inside (a, b): phi = S_fix + S_lin - W theta there
        const double r = (v[BUDGET_POINTS] + v[BUDGET_POINTS + 1] - budget) / v[BUDGET_POINTS + 2];
        *th = !isfinite(r) ? b0 : (r < a0 ? a0 : (r > b0 ? b0 : r));
        return true;
    }
    double lo = a0, hi = b0;
    for (int j = 1; j <= BUDGET_POINTS; ++j) {
        const double p = budget_point(a0, b0, j);
        if (!(v[j - 1] > budget)) { hi = p; break; }
        lo = p;
    }
    if (!(hi > lo) || (lo == a0 && hi == b0)) { *th = b0; return true; }     // the doubles between a and b are used up
    *a = lo;
    *b = hi;
    return false;
}

extern "C" {

int femfct_budget_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0, int32_t K,
                         double alpha, double budget, double c_lower, double c_upper, int32_t num_steps, double dt,
                         double* c_out_dev, double* src_out_dev, double* lambda_host, double* l1_host, int32_t* rounds_host) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->have_mass, "mass matrix not set");
    ARG_TRY(ctx, c_dev && c_out_dev && lambda_host && l1_host && rounds_host, "null argument");
    ARG_TRY(ctx, K >= 1 && K <= FEMFCT_MAX_TRIALS, "K (number of Armijo trials) must be in 1..16");
    ARG_TRY(ctx, d_dev || K == 1, "d may be NULL (the projection of c itself) only with K = 1");
    ARG_TRY(ctx, alpha >= 0.0 && isfinite(alpha), "alpha (L1 weight) must be >= 0 and finite");
    ARG_TRY(ctx, budget > 0.0 && isfinite(budget), "budget must be > 0 and finite");
    ARG_TRY(ctx, c_lower <= 0.0 && 0.0 <= c_upper, "the box must contain 0: c_lower <= 0 <= c_upper");
    ARG_TRY(ctx, num_steps >= 0, "num_steps must be >= 0");
    ARG_TRY(ctx, isfinite(s0) && isfinite(dt), "s0 and dt must be finite");
    const int levels = num_steps + 1;
    const int64_t items = (int64_t)levels * K;
    LaunchGeom g = femfct_geom(ctx, 1);
    const int G = g.grid.x;
    // rounds: 256-thread blocks of about 8 rows a thread
    int64_t Gr = ((int64_t)ctx->n + 2047) / 2048;
    if (Gr > FEMFCT_MAX_PARTIALS) Gr = FEMFCT_MAX_PARTIALS;
    const size_t pw = (size_t)items * G, pr = (size_t)items * Gr;
    int rc = femfct_ensure_scratch(ctx, 2 * pw + 2 * (size_t)K + (BUDGET_SUMS + 1) * pr + (size_t)BUDGET_VALS * K);
    if (rc != FEMFCT_OK) return rc;
    double *part_l = ctx->d_scratch, *part_m = part_l + pw, *out_w = part_m + pw;       // out_w: K norms, K maxima
    double *part_s = out_w + 2 * K, *part_c = part_s + BUDGET_SUMS * pr, *out_r = part_c + pr;   // out_r: K*18 sums, K counts

    double tau[FEMFCT_MAX_TRIALS], th[FEMFCT_MAX_TRIALS], vals[FEMFCT_MAX_TRIALS * BUDGET_VALS];
    for (int t = 0; t < K; ++t) {
        const double s = d_dev ? s0 * (1.0 / (double)(1 << t)) : 0.0;      // the kernels' expressions
        tau[t] = s * alpha;
    }
    auto write = [&](const BudgetWrite& par) -> int {
        g.grid.y = grid_y(items);
        hipLaunchKernelGGL(k_budget_write, g.grid, g.block, 0, ctx->stream, ctx->n, ctx->d_ml, c_dev, d_dev, g_dev, s0, alpha,
                           c_lower, c_upper, levels, items, par, c_out_dev, src_out_dev, part_l, part_m);
        femfct_enqueue_reduce_levels(ctx, K, levels, G, part_l, 1, dt, 0, out_w);       // femfct_l1_norm_Q's fold
        hipLaunchKernelGGL(k_budget_max_fold, dim3(K), dim3(256), 0, ctx->stream, (int64_t)levels * G, part_m, out_w + K);
        HIP_TRY(ctx, hipMemcpyAsync(vals, out_w, sizeof(double) * 2 * K, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int t = 0; t < 2 * K; ++t)
            if (!isfinite(vals[t]))
                return femfct_fail(ctx, FEMFCT_ERR_INVALID, "femfct_budget_trials: non-finite value in c or d (trial %d: norm %g, max |x| %g)",
                                   t % K, vals[t % K], vals[K + t % K]);
        for (int t = 0; t < K; ++t) l1_host[t] = vals[t];
        return FEMFCT_OK;
    };

    // every trial with lambda = 0: femfct_prox_trials' values, their norms phi_t(tau_t) and max |x_t|
    BudgetWrite wp;
    BudgetRound rp;
    for (int t = 0; t < FEMFCT_MAX_TRIALS; ++t) { wp.lam[t] = 0.0; wp.active[t] = t < K; rp.a[t] = rp.b[t] = 0.0; rp.active[t] = 0; }
    rc = write(wp);
    if (rc != FEMFCT_OK) return rc;
    int pending = 0;
    for (int t = 0; t < K; ++t) {
        lambda_host[t] = 0.0;
        rounds_host[t] = 0;
        rp.a[t] = tau[t];
        rp.b[t] = vals[K + t] > tau[t] ? vals[K + t] : tau[t];
        wp.active[t] = rp.active[t] = l1_host[t] > budget && rp.b[t] > rp.a[t];
        pending += rp.active[t];
    }
    if (!pending) return FEMFCT_OK;

    // the search: at most BUDGET_MAX_ROUNDS launches and read-backs, whatever comes back
    for (int round = 1; round <= BUDGET_MAX_ROUNDS && pending; ++round) {
        dim3 grid((unsigned)Gr, grid_y(items), 1);
        hipLaunchKernelGGL(k_budget_round, grid, dim3(256), 0, ctx->stream, ctx->n, ctx->d_ml, c_dev, d_dev, s0, c_lower,
                           c_upper, levels, items, rp, part_s, part_c);
        femfct_enqueue_reduce_levels(ctx, K * BUDGET_SUMS, levels, (int)Gr, part_s, 1, dt, 0, out_r);
        femfct_enqueue_reduce_levels(ctx, K, levels, (int)Gr, part_c, 0, 1.0, 0, out_r + K * BUDGET_SUMS);
        HIP_TRY(ctx, hipMemcpyAsync(vals, out_r, sizeof(double) * BUDGET_VALS * K, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int t = 0; t < K; ++t) {
            if (!rp.active[t]) continue;
            double v[BUDGET_VALS];
            for (int j = 0; j < BUDGET_SUMS; ++j) v[j] = vals[t * BUDGET_SUMS + j];
            v[BUDGET_SUMS] = vals[K * BUDGET_SUMS + t];
            rounds_host[t] = round;
            if (femfct_budget_narrow(&rp.a[t], &rp.b[t], v, budget, &th[t])) { rp.active[t] = 0; --pending; }
        }
    }
    for (int t = 0; t < K; ++t) {
        if (rp.active[t]) th[t] = rp.b[t];          // the round cap: the feasible end of the bracket
        if (wp.active[t]) {
            const double lam = th[t] - tau[t];
            wp.lam[t] = lambda_host[t] = lam > 0.0 ? lam : 0.0;
        }
    }
    return write(wp);      // the trials over budget again, with their lambda; the others' partials stand
}

}  // extern "C"
