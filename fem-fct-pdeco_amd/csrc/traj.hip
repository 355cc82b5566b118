// Forward / adjoint trajectory sweeps resident on one GPU.
//
// One time step = [assemble the step's flux matrix] -> [FCT step] -> [advance level];
// the whole sequence is captured once into a hipGraph and replayed num_steps times.
// The current time level lives in a device-side counter that the captured kernels
// read (VecRef), so the replayed graph needs no per-step host patching.
//
//   solid-body rotation + drift control
//     forward  /root/reference/advection_solidbody_FCT_PDECO_finaltime.py:175-193
//     adjoint  /root/reference/advection_solidbody_FCT_PDECO_finaltime.py:200-221
//              /root/reference/advection_solidbody_FCT_PDECO_alltime.py:232-259
#include "femfct_internal.h"
#include "device_utils.h"
#include "forms.h"
#include "traj_common.h"
#include "solidbody_op.h"

#include <algorithm>
#include <cmath>

int femfct_enqueue_step_ref(femfct_ctx* ctx, const double* A, const double* N, int32_t nshared, VecRef rhs,
                            int64_t rhs_bstride, VecRef u_n, int64_t u_bstride, double dt, VecRef u_out,
                            int64_t out_bstride, int32_t batch, int32_t budget);
int femfct_enqueue_ops_solidbody(femfct_ctx* ctx, const double* Arot, VecRef c_ref, int64_t c_bstride, double eps,
                                 double sigma, double rot_scale, double bx, double by, double* A, int32_t batch,
                                 int32_t levels = 1);

// Whether the tile step's first launch would take a pre-built low-order operator (femfct_enqueue_step_op: fused build,
// fused du/dt and Chebyshev-flux tail; no non-flux matrix in the solid-body sweeps).
static bool prebuild_low_wanted(const femfct_ctx* ctx, int32_t batch) {
    TilePlan tp;
    return ctx->prebuild_low && ctx->fuse_build && ctx->fuse_dudt && ctx->structured && ctx->implicit_cols && ctx->W == 7 &&
           ctx->solver != FEMFCT_SOLVER_BICGSTAB && !femfct_mesh_step_wanted(ctx, batch) && !femfct_tile4_wanted(ctx, batch) &&
           femfct_tile_plan(ctx, &tp, false, 0, batch) && !femfct_tile_big(ctx, tp) && femfct_cheb_flux_fusable(ctx, batch);
}

// The solid-body operator depends on the control only, which is given for the whole sweep: assemble the
// matrices of all time levels in one launch before the sweep (HBM is large: Nt * 7n doubles per control
// trajectory, 92 MB at C2) instead of one small dependent launch per step.  Returns false (per-step
// assembly) when the sequence would not fit the configured cap or the launch grid.
// So does the low-order operator L_k = M_L + dt (A_k - D_k), D_k of the latency-regime tile step: built from the
// sequence by a second launch (2 x 92 MB more at C2, under the same cap) unless FEMFCT_PREBUILD_LOW=0; without it
// (or without room for it) the step's first launch builds them as before.
static bool solidbody_preassemble(femfct_ctx* ctx, const double* Arot, const double* c_traj, int32_t c_shared,
                                  int64_t tstride, int32_t c_level0, double eps, double sigma, double rot_scale, double bx,
                                  double by, int32_t num_steps, int32_t batch, double dt, MatRef* out) {
    const int32_t members = c_shared ? 1 : batch;
    const size_t count = (size_t)members * num_steps * ctx->W * ctx->n;
    ctx->low_src = nullptr;     // d_trAall is about to change: no pre-built L / D matches it
    if (!ctx->preassemble || (double)count * 8.0 > ctx->preassemble_max_bytes) return false;
    if ((int64_t)members * num_steps > 65535) return false;
    if (count > ctx->trAall_count) {
        femfct_drop_graphs(ctx);
        if (ctx->d_trAall) hipFree(ctx->d_trAall);
        ctx->d_trAall = nullptr; ctx->trAall_count = 0;
        if (hipMalloc((void**)&ctx->d_trAall, sizeof(double) * count) != hipSuccess) { (void)hipGetLastError(); return false; }
        ctx->trAall_count = count;
    }
    const int64_t n = ctx->n;
    femfct_enqueue_ops_solidbody(ctx, Arot, make_ref(c_traj, nullptr, n, c_level0), c_shared ? 0 : tstride, eps, sigma,
                                 rot_scale, bx, by, ctx->d_trAall, members, num_steps);
    const int64_t wn = (int64_t)ctx->W * n;
    *out = MatRef{ctx->d_trAall, ctx->d_level, wn, 0, c_shared ? 0 : wn * num_steps};
    if (prebuild_low_wanted(ctx, batch) && (double)count * 3.0 * 8.0 <= ctx->preassemble_max_bytes) {
        if (2 * count > ctx->lowall_count) {
            femfct_drop_graphs(ctx);
            if (ctx->d_lowall) hipFree(ctx->d_lowall);
            ctx->d_lowall = nullptr; ctx->lowall_count = 0;
            if (hipMalloc((void**)&ctx->d_lowall, sizeof(double) * 2 * count) != hipSuccess) (void)hipGetLastError();
            else ctx->lowall_count = 2 * count;
        }
        if (ctx->d_lowall &&
            femfct_enqueue_low_seq(ctx, ctx->d_trAall, ctx->d_lowall, ctx->d_lowall + count, members * num_steps, dt) == FEMFCT_OK) {
            ctx->low_src = ctx->d_trAall;
            ctx->low_dt = dt;
            ctx->low_doff = count;
        }
    }
    return true;
}
int femfct_enqueue_mass_diff(femfct_ctx* ctx, VecRef a, int64_t a_bstride, VecRef b, int64_t b_bstride, double* out,
                             int32_t batch);
int femfct_enqueue_axpby(femfct_ctx* ctx, int64_t count, double alpha, const double* a, double beta, const double* b,
                         double* out);

namespace {

// end of a step: log the solver control blocks, then move the level counter
__global__ void k_step_end(int32_t* level, int delta, int ord_adv, int ord_off, const StepCtl* __restrict__ ctl,
                           StepCtl* __restrict__ log, const KrylovCtl* __restrict__ kctl, KrylovCtl* __restrict__ klog,
                           int batch) {
    const int ord = level[1];
    for (int b = threadIdx.x; b < batch; b += blockDim.x) {
        log[(int64_t)(ord + ord_off) * batch + b] = ctl[b];
        if (kctl) klog[(int64_t)(ord + ord_off) * batch + b] = kctl[b];
    }
    __syncthreads();
    if (threadIdx.x == 0 && ord_adv) {      // the last step of a graph moves the counters for all of its steps
        level[0] += delta;
        level[1] = ord + ord_adv;
    }
}

}  // namespace

// The FCT step is the last operation of this kind of time step: let its final kernel log and advance.
void femfct_request_fused_end(femfct_ctx* ctx, int delta, bool with_krylov) {
    ctx->end_req_delta = ctx->fuse_end ? delta : 0;
    ctx->end_req_krylov = with_krylov;
    ctx->end_fused = false;
}

int femfct_enqueue_step_end(femfct_ctx* ctx, int delta, int32_t batch, bool with_krylov) {
    ctx->end_req_delta = 0;
    if (ctx->end_fused) {   // already done by the step's last kernel
        ctx->end_fused = false;
        return FEMFCT_OK;
    }
    hipLaunchKernelGGL(k_step_end, dim3(1), dim3(64), 0, ctx->stream, ctx->d_level, ctx->rep_last ? delta * ctx->rep_total : 0,
                       ctx->rep_last ? ctx->rep_total : 0, ctx->ord_bias, ctx->d_ctl, ctx->d_log,
                       with_krylov ? (const KrylovCtl*)ctx->d_kry_ctl : nullptr, (KrylovCtl*)ctx->d_klog, batch);
    return FEMFCT_OK;
}

int femfct_ensure_traj_ws(femfct_ctx* ctx, int32_t batch, int32_t steps) {
    int rc = femfct_ensure_workspace(ctx, batch);
    if (rc != FEMFCT_OK) return rc;
    if (batch > ctx->tr_batch) {
        femfct_drop_graphs(ctx);
        if (ctx->d_trA) hipFree(ctx->d_trA);
        if (ctx->d_trN) hipFree(ctx->d_trN);
        if (ctx->d_trRhs) hipFree(ctx->d_trRhs);
        ctx->d_trA = ctx->d_trN = ctx->d_trRhs = nullptr;
        size_t nv = (size_t)batch * ctx->n, nm = nv * ctx->W;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trA, sizeof(double) * nm));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trN, sizeof(double) * nm));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trRhs, sizeof(double) * nv));
        for (double** q : {&ctx->d_trMat, &ctx->d_trBase, &ctx->d_trBase2, &ctx->d_trRhs2, &ctx->d_trTmp}) {
            if (*q) hipFree(*q);
            *q = nullptr;
        }
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trMat, sizeof(double) * nm));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trBase, sizeof(double) * ctx->W * ctx->n));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trBase2, sizeof(double) * ctx->W * ctx->n));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trRhs2, sizeof(double) * nv));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_trTmp, sizeof(double) * nv));
        if (ctx->d_log) hipFree(ctx->d_log);
        ctx->d_log = nullptr;
        ctx->tr_steps = 0;
        ctx->tr_batch = batch;
    }
    if (!ctx->d_level) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_level, sizeof(int32_t) * 2));
    if (!ctx->d_ticket) {
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_ticket, sizeof(unsigned)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_ticket, 0, sizeof(unsigned), ctx->stream));
    }
    if (steps > ctx->tr_steps || !ctx->d_log) {
        femfct_drop_graphs(ctx);
        if (ctx->d_log) hipFree(ctx->d_log);
        ctx->d_log = nullptr;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_log, sizeof(StepCtl) * (size_t)steps * ctx->tr_batch));
        if (ctx->d_klog) hipFree(ctx->d_klog);
        ctx->d_klog = nullptr;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_klog, sizeof(KrylovCtl) * (size_t)steps * ctx->tr_batch));
        ctx->tr_steps = steps;
    }
    return FEMFCT_OK;
}

// the same sweep with a source trajectory: rhs_{n+1} = assemble(src_{n+1} * v * dx) = M src_{n+1}
// (advection_FCT_PDECO_alltime_exact.py:249-253: u_rhs = assemble((g_np1 + c_np1)*v*dx), A_u = A - eps*Ad)
// g_traj (may be null): coefficient trajectory of an explicit reaction term, shared by the batch:
// rhs_{n+1} = M src_{n+1} - Mg(g_n) u_n in one launch (advection_FCT_PDECO_finaltime_exact.py:273-277)
static int solidbody_forward_sweep(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                   const double* src_traj, const double* g_traj, double* u_traj, int32_t num_steps,
                                   double dt, double eps, double rot_scale, double bx, double by, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, c_traj && u_traj && num_steps >= 1 && dt > 0 && batch >= 1, "bad argument");
    ARG_TRY(ctx, Arot_ell || rot_scale == 0.0, "Arot_ell is required when rot_scale != 0");
    int rc = femfct_ensure_traj_ws(ctx, batch, num_steps);
    if (rc != FEMFCT_OK) return rc;
    const int64_t n = ctx->n, tstride = (int64_t)(num_steps + 1) * n;
    const double* Arot = Arot_ell ? Arot_ell : ctx->d_Ad;  // any valid ELL array; multiplied by 0
    int32_t* lv = ctx->d_level;
    MatRef Aall{};
    bool pre = false;
    // step k (level counter k) uses the control of level k+1 (finaltime.py:185): sequence entry k
    // bandwidth regime: the step kernels derive the operator from Arot and the control themselves (no stored A)
    bool inl = false;
    int rotg = 0;
    double rot_om = 0.0;
    auto begin = [&]() {
        inl = femfct_inline_ops_wanted(ctx, batch);     // (inside the sweep driver: depends on the kind's Jacobi kernel)
        rotg = inl && Arot_ell && rot_scale != 0.0 && femfct_rotation_is_geometric(ctx, Arot, &rot_om);
        ctx->last_rot_geom = rotg != 0;
        if (!inl)
            pre = solidbody_preassemble(ctx, Arot, c_traj, c_shared, tstride, 1, eps, -1.0, rot_scale, bx, by, num_steps,
                                        batch, dt, &Aall);
        return FEMFCT_OK;
    };
    auto step = [&](int budget, int, int reps) {
        femfct_ctx::GraphKey key{(uint64_t)SWEEP_SOLIDBODY_FORWARD, key_bits(Arot), key_bits(c_traj), key_bits(c_shared), key_bits(u_traj),
                                 key_bits(num_steps), key_bits(dt), key_bits(eps), key_bits(rot_scale), key_bits(bx),
                                 key_bits(by), key_bits(batch), key_bits((int32_t)budget), key_bits(ctx->rel_tol),
                                 key_bits(pre ? Aall.base : nullptr), key_bits(src_traj), key_bits((int32_t)inl),
                                 key_bits((int32_t)rotg), key_bits(rot_om), key_bits(g_traj)};
        return femfct_run_graph_reps(ctx, key, reps, +1, [&]() {
            // control at level n+1 (finaltime.py:185), state from level n into level n+1
            MatRef A = Aall;
            if (A.level) A.level_off += ctx->level_bias;
            const SbOpArgs sb{Arot, ctx->d_Ad, lref(ctx, c_traj, lv, n, 1), c_shared ? 0 : tstride, eps, -1.0, rot_scale, bx, by,
                              rotg, rot_om, ctx->a1};
            if (!pre && !inl) {
                femfct_enqueue_ops_solidbody(ctx, Arot, lref(ctx, c_traj, lv, n, 1), c_shared ? 0 : tstride, eps, -1.0,
                                             rot_scale, bx, by, ctx->d_trA, batch);
                A = MatRef{ctx->d_trA, nullptr, 0, 0, (int64_t)ctx->W * n};
            }
            VecRef rhs = make_ref(nullptr);
            if (g_traj) {       // source at level n+1, coefficient and state at level n
                ReactLoadSpec rl;
                rl.a = lref(ctx, src_traj, lv, n, 1); rl.a_bs = tstride;
                rl.g = lref(ctx, g_traj, lv, n, 0);   rl.g_bs = 0;
                rl.x = lref(ctx, u_traj, lv, n, 0);   rl.x_bs = tstride;
                femfct_enqueue_react_load(ctx, rl, ctx->d_trRhs, batch);
                rhs = make_ref(ctx->d_trRhs);
            } else if (src_traj) {
                femfct_enqueue_mass_diff(ctx, lref(ctx, src_traj, lv, n, 1), tstride, make_ref(nullptr), 0, ctx->d_trRhs, batch);
                rhs = make_ref(ctx->d_trRhs);
            }
            femfct_request_fused_end(ctx, 1, false);
            int r = femfct_enqueue_step_op(ctx, A, inl ? &sb : nullptr, nullptr, 0, rhs, n,
                                           lref(ctx, u_traj, lv, n, 0), tstride, dt, lref(ctx, u_traj, lv, n, 1),
                                           tstride, batch, budget);
            if (r != FEMFCT_OK) return r;
            femfct_enqueue_step_end(ctx, 1, batch, false);
            return FEMFCT_OK;
        });
    };
    // (a diffusive operator has no upwind rows: no point in finding that out from a whole sweep with the pair-compact launch;
    // nor has the operator of a sweep with a reaction term, whose adjoint carries a mass-like part)
    return femfct_run_sweep(ctx, SweepSpec{SWEEP_SOLIDBODY_FORWARD, num_steps, batch, 0, false, g_traj || eps != 0.0}, begin, step);
}

// Snapshot tracking (kernels_obs.hip): J = 1/2 sum_n theta_n ||u_n - uhat_n||^2_Mw + tau/2 ||u_Nt - uhat_Nt||^2.  theta:
// num_steps + 1 weights on the device, read per level through the level counter; window (may be null): nodal omega >= 0.
struct ObsArgs {
    const double* theta;
    double tau;
    const double* window;
};

// State bounds as a Moreau-Yosida penalty on top of the tracking (kernels_bounds.hip; needs obs): lower / upper (either
// may be null) and window_s: n doubles on the device, sigma: num_steps + 1 level weights on the device.
struct BoundArgs {
    const double *lower, *upper;
    double gamma;
    const double *sigma, *window_s;
};

// g_traj (may be null): rhs_n = [M (uhat_n - u_n)] - Mg(g_n) p_{n+1}, the coefficient at the level being produced
// (advection_FCT_PDECO_finaltime_exact.py:317-321); the final-time sweep has a right-hand side then, too
// obs (may be null; `alltime` is unused with it): uhat is a trajectory, p_Nt = tau omega (uhat_Nt - u_Nt) and
// rhs_n = (theta_n/dt) Mw (uhat_n - u_n) [- Mg(g_n) p_{n+1}]: the two modes above are (tau, theta) = (1, 0) and (0, dt)
static int solidbody_adjoint_sweep(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                   const double* g_traj, const double* u_traj, const double* uhat, double* p_traj,
                                   int32_t num_steps, double dt, double eps, double rot_scale, double bx, double by,
                                   int32_t alltime, int32_t batch, const ObsArgs* obs = nullptr,
                                   const BoundArgs* bnd = nullptr) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, c_traj && u_traj && uhat && p_traj && num_steps >= 1 && dt > 0 && batch >= 1, "bad argument");
    ARG_TRY(ctx, !obs || obs->theta, "theta is null");
    ARG_TRY(ctx, !obs || obs->tau >= 0.0, "tau must be >= 0");
    ARG_TRY(ctx, !bnd || obs, "state bounds need observations");
    ARG_TRY(ctx, !bnd || bnd->sigma, "sigma is null");
    ARG_TRY(ctx, !bnd || bnd->lower || bnd->upper, "no bound: lower and upper are both null");
    ARG_TRY(ctx, !bnd || (bnd->gamma >= 0.0 && std::isfinite(bnd->gamma)), "gamma must be finite and >= 0");
    ARG_TRY(ctx, Arot_ell || rot_scale == 0.0, "Arot_ell is required when rot_scale != 0");
    int rc = femfct_ensure_traj_ws(ctx, batch, num_steps);
    if (rc != FEMFCT_OK) return rc;
    const int64_t n = ctx->n, tstride = (int64_t)(num_steps + 1) * n;
    const double* Arot = Arot_ell ? Arot_ell : ctx->d_Ad;
    int32_t* lv = ctx->d_level;
    MatRef Aall{};
    bool pre = false;
    bool inl = false;
    int rotg = 0;
    double rot_om = 0.0;
    auto begin = [&]() {
        inl = femfct_inline_ops_wanted(ctx, batch);
        rotg = inl && Arot_ell && rot_scale != 0.0 && femfct_rotation_is_geometric(ctx, Arot, &rot_om);
        ctx->last_rot_geom = rotg != 0;
        // level counter n uses the control of level n (finaltime.py:213): sequence entry n
        if (!inl)
            pre = solidbody_preassemble(ctx, Arot, c_traj, c_shared, tstride, 0, eps, +1.0, rot_scale, bx, by, num_steps,
                                        batch, dt, &Aall);
        // terminal condition: p(T) = uhat_T - u(T) (finaltime.py:201) or 0 (alltime.py:232)
        if (obs) {      // p(T) = tau omega (uhat_T - u(T)); tau = 0: uhat_T is not read
            double* pT = p_traj + (int64_t)num_steps * n;
            if (bnd)    // ... - sigma_Nt gamma window_s .* v_Nt
                femfct_enqueue_bound_terminal(ctx, obs->tau, obs->window, uhat + (int64_t)num_steps * n, tstride,
                                              u_traj + (int64_t)num_steps * n, tstride, bnd->sigma + num_steps, bnd->gamma,
                                              bnd->lower, bnd->upper, bnd->window_s, pT, tstride, batch);
            else if (obs->tau == 0.0)
                for (int32_t b = 0; b < batch; ++b) HIP_TRY(ctx, hipMemsetAsync(pT + b * tstride, 0, sizeof(double) * n, ctx->stream));
            else
                femfct_enqueue_obs_terminal(ctx, obs->tau, obs->window, uhat + (int64_t)num_steps * n, tstride,
                                            u_traj + (int64_t)num_steps * n, tstride, pT, tstride, batch);
            return FEMFCT_OK;
        }
        for (int32_t b = 0; b < batch; ++b) {
            double* pT = p_traj + b * tstride + (int64_t)num_steps * n;
            if (alltime) HIP_TRY(ctx, hipMemsetAsync(pT, 0, sizeof(double) * n, ctx->stream));
            else femfct_enqueue_axpby(ctx, n, 1.0, uhat + (int64_t)b * n, -1.0, u_traj + b * tstride + (int64_t)num_steps * n, pT);
        }
        return FEMFCT_OK;
    };
    auto step = [&](int budget, int, int reps) {
        femfct_ctx::GraphKey key{(uint64_t)SWEEP_SOLIDBODY_ADJOINT, key_bits(Arot), key_bits(c_traj), key_bits(c_shared), key_bits(u_traj),
                                 key_bits(uhat), key_bits(p_traj), key_bits(num_steps), key_bits(dt), key_bits(eps),
                                 key_bits(rot_scale), key_bits(bx), key_bits(by), key_bits(alltime), key_bits(batch),
                                 key_bits((int32_t)budget), key_bits(ctx->rel_tol), key_bits(pre ? Aall.base : nullptr),
                                 key_bits((int32_t)inl), key_bits((int32_t)rotg), key_bits(rot_om), key_bits(g_traj)};
        if (obs) {      // another load kernel is captured, with these arguments
            key.push_back(key_bits(obs->theta));
            key.push_back(key_bits(obs->tau));
            key.push_back(key_bits(obs->window));
            key.push_back(key_bits((int32_t)1));
        }
        if (bnd) {      // the load kernel with the penalty term: its arguments are baked into the graph, gamma too
            key.push_back(key_bits(bnd->lower));
            key.push_back(key_bits(bnd->upper));
            key.push_back(key_bits(bnd->gamma));
            key.push_back(key_bits(bnd->sigma));
            key.push_back(key_bits(bnd->window_s));
            key.push_back(key_bits((int32_t)2));
        }
        return femfct_run_graph_reps(ctx, key, reps, -1, [&]() {
            // level counter = n: control c_n (finaltime.py:213), p_{n+1} -> p_n
            MatRef A = Aall;
            if (A.level) A.level_off += ctx->level_bias;
            const SbOpArgs sb{Arot, ctx->d_Ad, lref(ctx, c_traj, lv, n, 0), c_shared ? 0 : tstride, eps, +1.0, rot_scale, bx, by,
                              rotg, rot_om, ctx->a1};
            if (!pre && !inl) {
                femfct_enqueue_ops_solidbody(ctx, Arot, lref(ctx, c_traj, lv, n, 0), c_shared ? 0 : tstride, eps, +1.0,
                                             rot_scale, bx, by, ctx->d_trA, batch);
                A = MatRef{ctx->d_trA, nullptr, 0, 0, (int64_t)ctx->W * n};
            }
            VecRef rhs = make_ref(nullptr);
            if (obs) {      // the weighted misfit of level n (and the reaction term) in the load launch of the all-time step
                ObsLoadSpec ol;
                ol.a = lref(ctx, uhat, lv, n, 0);   ol.a_bs = tstride;
                ol.b = lref(ctx, u_traj, lv, n, 0); ol.b_bs = tstride;
                ol.theta = lref(ctx, obs->theta, lv, 1, 0);
                ol.w = make_ref(obs->window);
                ol.dt = dt;
                if (g_traj) {
                    ol.g = lref(ctx, g_traj, lv, n, 0);
                    ol.x = lref(ctx, p_traj, lv, n, 1); ol.x_bs = tstride;
                }
                if (bnd) {
                    BoundSpec bs;
                    bs.sigma = lref(ctx, bnd->sigma, lv, 1, 0);
                    bs.u = lref(ctx, u_traj, lv, n, 0); bs.u_bs = tstride;
                    bs.lo = bnd->lower; bs.hi = bnd->upper; bs.ml = ctx->d_ml; bs.ws = bnd->window_s;
                    bs.gamma = bnd->gamma;
                    femfct_enqueue_bound_load(ctx, ol, bs, ctx->d_trRhs, batch);
                } else {
                    femfct_enqueue_obs_load(ctx, ol, ctx->d_trRhs, batch);
                }
                rhs = make_ref(ctx->d_trRhs);
            } else if (g_traj) {   // coefficient at level n, adjoint at level n+1; all-time: the misfit load in the same launch
                ReactLoadSpec rl;
                if (alltime) {
                    rl.a = lref(ctx, uhat, lv, n, 0);   rl.a_bs = tstride;
                    rl.b = lref(ctx, u_traj, lv, n, 0); rl.b_bs = tstride;
                }
                rl.g = lref(ctx, g_traj, lv, n, 0); rl.g_bs = 0;
                rl.x = lref(ctx, p_traj, lv, n, 1); rl.x_bs = tstride;
                femfct_enqueue_react_load(ctx, rl, ctx->d_trRhs, batch);
                rhs = make_ref(ctx->d_trRhs);
            } else if (alltime) {  // rhs = assemble((uhat_n - u_n) v dx)  (alltime.py:257)
                femfct_enqueue_mass_diff(ctx, lref(ctx, uhat, lv, n, 0), tstride, lref(ctx, u_traj, lv, n, 0), tstride,
                                         ctx->d_trRhs, batch);
                rhs = make_ref(ctx->d_trRhs);
            }
            femfct_request_fused_end(ctx, -1, false);
            int r = femfct_enqueue_step_op(ctx, A, inl ? &sb : nullptr, nullptr, 0, rhs, n, lref(ctx, p_traj, lv, n, 1), tstride,
                                           dt, lref(ctx, p_traj, lv, n, 0), tstride, batch, budget);
            if (r != FEMFCT_OK) return r;
            femfct_enqueue_step_end(ctx, -1, batch, false);
            return FEMFCT_OK;
        });
    };
    return femfct_run_sweep(ctx, SweepSpec{SWEEP_SOLIDBODY_ADJOINT, num_steps, batch, num_steps - 1, false, g_traj || eps != 0.0}, begin, step);
}

// the zero drift control of the linear sweeps (the control enters through the source): (num_steps + 1) * n zeros
static int zero_control(femfct_ctx* ctx, int32_t num_steps, const double** out) {
    const size_t count = (size_t)(num_steps + 1) * ctx->n;
    if (count > ctx->zero_traj_count) {
        femfct_drop_graphs(ctx);
        if (ctx->d_zero_traj) hipFree(ctx->d_zero_traj);
        ctx->d_zero_traj = nullptr; ctx->zero_traj_count = 0;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_zero_traj, sizeof(double) * count));
        ctx->zero_traj_count = count;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_zero_traj, 0, sizeof(double) * count, ctx->stream));
    }
    *out = ctx->d_zero_traj;
    return FEMFCT_OK;
}

extern "C" {

int femfct_solidbody_forward(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                             double* u_traj, int32_t num_steps, double dt, double eps, double rot_scale, double bx,
                             double by, int32_t batch) {
    return femfct_solidbody_forward_src(ctx, Arot_ell, c_traj, c_shared, nullptr, u_traj, num_steps, dt, eps, rot_scale, bx,
                                        by, batch);
}

int femfct_solidbody_forward_src(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                 const double* src_traj, double* u_traj, int32_t num_steps, double dt, double eps,
                                 double rot_scale, double bx, double by, int32_t batch) {
    return solidbody_forward_sweep(ctx, Arot_ell, c_traj, c_shared, src_traj, nullptr, u_traj, num_steps, dt, eps, rot_scale,
                                   bx, by, batch);
}

int femfct_solidbody_adjoint(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                             const double* u_traj, const double* uhat, double* p_traj, int32_t num_steps, double dt,
                             double eps, double rot_scale, double bx, double by, int32_t alltime, int32_t batch) {
    return solidbody_adjoint_sweep(ctx, Arot_ell, c_traj, c_shared, nullptr, u_traj, uhat, p_traj, num_steps, dt, eps,
                                   rot_scale, bx, by, alltime, batch);
}

// Linear advection-diffusion-reaction, du/dt - eps lap u + div(w u) + g u = src, the reaction term explicit:
// advection_FCT_PDECO_finaltime_exact.py:252-279 (state), :344-370 (sensitivity: src = d, zero initial condition)
int femfct_linear_forward_react(femfct_ctx* ctx, const double* A_ell, const double* src_traj, const double* g_traj,
                                double* u_traj, int32_t num_steps, double dt, double eps, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, A_ell && g_traj && u_traj && num_steps >= 1 && batch >= 1, "bad argument");
    const double* zc = nullptr;
    int rc = zero_control(ctx, num_steps, &zc);
    if (rc != FEMFCT_OK) return rc;
    return solidbody_forward_sweep(ctx, A_ell, zc, 1, src_traj, g_traj, u_traj, num_steps, dt, eps, 1.0, 0.0, 0.0, batch);
}

// its adjoint, :293-322: A_p = -Aadj - eps*Ad with Aadj = Aa1 + Aa2 given
int femfct_linear_adjoint_react(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                const double* uhat, double* p_traj, int32_t num_steps, double dt, double eps,
                                int32_t alltime, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, Aadj_ell && g_traj && u_traj && uhat && p_traj && num_steps >= 1 && batch >= 1, "bad argument");
    const double* zc = nullptr;
    int rc = zero_control(ctx, num_steps, &zc);
    if (rc != FEMFCT_OK) return rc;
    return solidbody_adjoint_sweep(ctx, Aadj_ell, zc, 1, g_traj, u_traj, uhat, p_traj, num_steps, dt, eps, 1.0, 0.0, 0.0,
                                   alltime, batch);
}

// Adjoint sweeps that track the state at chosen time levels (snapshot observations; added after ABI version 5, backward
// compatible): see ObsArgs.  (tau, theta) = (1, 0) and (0, dt) enqueue the arithmetic of alltime = 0 and 1.
int femfct_solidbody_adjoint_obs(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                 const double* u_traj, const double* uhat_traj, const double* theta, double tau,
                                 const double* window, double* p_traj, int32_t num_steps, double dt, double eps,
                                 double rot_scale, double bx, double by, int32_t batch) {
    const ObsArgs obs{theta, tau, window};
    return solidbody_adjoint_sweep(ctx, Arot_ell, c_traj, c_shared, nullptr, u_traj, uhat_traj, p_traj, num_steps, dt, eps,
                                   rot_scale, bx, by, 0, batch, &obs);
}

int femfct_linear_adjoint_react_obs(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                    const double* uhat_traj, const double* theta, double tau, const double* window,
                                    double* p_traj, int32_t num_steps, double dt, double eps, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, theta, "theta is null");
    ARG_TRY(ctx, Aadj_ell && g_traj && u_traj && uhat_traj && p_traj && num_steps >= 1 && batch >= 1, "bad argument");
    const double* zc = nullptr;
    int rc = zero_control(ctx, num_steps, &zc);
    if (rc != FEMFCT_OK) return rc;
    const ObsArgs obs{theta, tau, window};
    return solidbody_adjoint_sweep(ctx, Aadj_ell, zc, 1, g_traj, u_traj, uhat_traj, p_traj, num_steps, dt, eps, 1.0, 0.0, 0.0,
                                   0, batch, &obs);
}

// The snapshot sweeps with state bounds lower <= u_n <= upper as a Moreau-Yosida penalty (BoundArgs, kernels_bounds.hip;
// added after ABI version 5, backward compatible)
int femfct_solidbody_adjoint_bounds(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                    const double* u_traj, const double* uhat_traj, const double* theta, double tau,
                                    const double* window, const double* lower, const double* upper, double gamma,
                                    const double* sigma, const double* window_s, double* p_traj, int32_t num_steps,
                                    double dt, double eps, double rot_scale, double bx, double by, int32_t batch) {
    const ObsArgs obs{theta, tau, window};
    const BoundArgs bnd{lower, upper, gamma, sigma, window_s};
    return solidbody_adjoint_sweep(ctx, Arot_ell, c_traj, c_shared, nullptr, u_traj, uhat_traj, p_traj, num_steps, dt, eps,
                                   rot_scale, bx, by, 0, batch, &obs, &bnd);
}

int femfct_linear_adjoint_react_bounds(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                       const double* uhat_traj, const double* theta, double tau, const double* window,
                                       const double* lower, const double* upper, double gamma, const double* sigma,
                                       const double* window_s, double* p_traj, int32_t num_steps, double dt, double eps,
                                       int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && ctx->structured, "structured mesh not set (femfct_set_mesh_square)");
    ARG_TRY(ctx, theta, "theta is null");
    ARG_TRY(ctx, Aadj_ell && g_traj && u_traj && uhat_traj && p_traj && num_steps >= 1 && batch >= 1, "bad argument");
    const double* zc = nullptr;
    int rc = zero_control(ctx, num_steps, &zc);
    if (rc != FEMFCT_OK) return rc;
    const ObsArgs obs{theta, tau, window};
    const BoundArgs bnd{lower, upper, gamma, sigma, window_s};
    return solidbody_adjoint_sweep(ctx, Aadj_ell, zc, 1, g_traj, u_traj, uhat_traj, p_traj, num_steps, dt, eps, 1.0, 0.0, 0.0,
                                   0, batch, &obs, &bnd);
}

// per-step solver diagnostics of the most recent trajectory sweep: info[step*batch + b]
int femfct_traj_info(femfct_ctx* ctx, femfct_step_info* info_host, int32_t num_steps, int32_t batch) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx && info_host, "null argument");
    ARG_TRY(ctx, num_steps == ctx->log_steps && batch == ctx->log_batch, "no matching trajectory log");
    for (size_t k = 0; k < ctx->h_log.size(); ++k) {
        info_host[k].flags = ctx->h_log[k].flags;
        info_host[k].solver_iters = ctx->h_log[k].iters;
        info_host[k].solver_resid = ctx->h_log[k].resid;
        info_host[k].min_rowsum = ctx->h_log[k].min_rowsum;
    }
    return FEMFCT_OK;
}

}  // extern "C"
