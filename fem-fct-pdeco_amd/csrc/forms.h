// Argument structs of the quadrature-form kernels (kernels_forms.hip) and the Krylov solver.
#pragma once

#include "device_utils.h"

struct femfct_ctx;

struct MeshArgs {
    int n, N, nc;
    double h;
    const int32_t* d2v;
    const int32_t* cols;
    const double* M;
    const double* Ad;
};

// out = alpha*M + gamma*base + beta * int f1 f2 phi_i phi_j
struct WMassSpec {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
    const double* base = nullptr;   // constant ELL matrix (shared by the batch)
    VecRef f1{nullptr, nullptr, 0, 0}, f2{nullptr, nullptr, 0, 0};
    int64_t f1_bs = 0, f2_bs = 0;
};

// out_i = s0*(M mx)_i + s1 * int (k0 + k1*p1 + k2*q1*q2*q3) phi_i + s2*(da_i - db_i) + s3*(M (ea - eb))_i
struct LoadSpec {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, k0 = 0.0, k1 = 0.0, k2 = 0.0;
    VecRef mx{nullptr, nullptr, 0, 0}, p1{nullptr, nullptr, 0, 0}, q1{nullptr, nullptr, 0, 0},
        q2{nullptr, nullptr, 0, 0}, q3{nullptr, nullptr, 0, 0}, da{nullptr, nullptr, 0, 0},
        db{nullptr, nullptr, 0, 0}, ea{nullptr, nullptr, 0, 0}, eb{nullptr, nullptr, 0, 0};
    int64_t mx_bs = 0, p1_bs = 0, q1_bs = 0, q2_bs = 0, q3_bs = 0, da_bs = 0, db_bs = 0, ea_bs = 0, eb_bs = 0;
};

// out_i = (M (a - b))_i - sum_j (int g_h phi_i phi_j) x_j   (kernels_react.hip; a absent: no mass term, b absent: M a)
struct ReactLoadSpec {
    VecRef a{nullptr, nullptr, 0, 0}, b{nullptr, nullptr, 0, 0}, g{nullptr, nullptr, 0, 0}, x{nullptr, nullptr, 0, 0};
    int64_t a_bs = 0, b_bs = 0, g_bs = 0, x_bs = 0;
};

// out = (theta/dt) * Mw(w) (a - b) - Mg(g) x   (kernels_obs.hip: the load of an adjoint step that tracks snapshots;
// theta: the level's weight, read on the device; w absent: Mw = M; g absent: no reaction term; g, w shared by the batch)
struct ObsLoadSpec {
    VecRef a{nullptr, nullptr, 0, 0}, b{nullptr, nullptr, 0, 0}, theta{nullptr, nullptr, 0, 0}, w{nullptr, nullptr, 0, 0},
        g{nullptr, nullptr, 0, 0}, x{nullptr, nullptr, 0, 0};
    int64_t a_bs = 0, b_bs = 0, x_bs = 0;
    double dt = 1.0;
};

// State bounds lo <= u <= hi as a Moreau-Yosida penalty (kernels_bounds.hip): what the load of an adjoint step loses,
//   (sigma/dt) * gamma * ml_i * ws_i * v_i,    v = u - clip(u, lo, hi),
// sigma: the level's weight, read on the device; sigma == 0: u is not read.  lo / hi absent: no bound on that side; ws
// (a nodal window) absent: 1.  lo, hi, ml, ws are shared by the batch.
struct BoundSpec {
    VecRef sigma{nullptr, nullptr, 0, 0}, u{nullptr, nullptr, 0, 0};
    int64_t u_bs = 0;
    const double *lo = nullptr, *hi = nullptr, *ml = nullptr, *ws = nullptr;
    double gamma = 0.0;
};

// out_i = s1 * int q1 q2 phi_i + s2*(da_i - db_i) + int (g0 + g1*a + g2*a^2) a^e b phi_i   (kernels_growth.hip: the growth
// term of the chemotaxis system; b absent: 1, q1 / da absent: no such term)
struct GrowthLoadSpec {
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, s1 = 0.0, s2 = 0.0;
    int e = 0;
    VecRef a{nullptr, nullptr, 0, 0}, b{nullptr, nullptr, 0, 0}, q1{nullptr, nullptr, 0, 0}, q2{nullptr, nullptr, 0, 0},
        da{nullptr, nullptr, 0, 0}, db{nullptr, nullptr, 0, 0};
    int64_t a_bs = 0, b_bs = 0, q1_bs = 0, q2_bs = 0, da_bs = 0, db_bs = 0;
};

// The misfit a snapshot sweep of the three PDE systems adds to a load of its adjoint step (ObsTail, forms_device.h), in the
// launch that assembles that load:
//   out_i += pre * (theta/dt) * (Mw(w) (a - b))_i   (mass)      or      out_i += pre * (theta/dt) * w_i (a_i - b_i)   (nodal)
// theta: the level's weight, read on the device through the level counter; theta == 0: a and b are not read.  theta
// absent: no term (the variable is not observed).  w absent: no window (Mw = M, w = 1); w is shared by the batch.
struct ObsTerm {
    VecRef theta{nullptr, nullptr, 0, 0}, a{nullptr, nullptr, 0, 0}, b{nullptr, nullptr, 0, 0}, w{nullptr, nullptr, 0, 0};
    int64_t a_bs = 0, b_bs = 0;
    double pre = 1.0, dt = 1.0;
    int mass = 1;
};

// up to three independent forms of a time step in one launch (kernels_forms.hip: k_forms2 / k_forms3)
enum { FORM_NONE = 0, FORM_WMASS, FORM_LOAD, FORM_CHTXS_MAT0, FORM_CHTXS_MAT1 };
struct ChtxsMatSpec {
    VecRef u{nullptr, nullptr, 0, 0}, v{nullptr, nullptr, 0, 0};
    int64_t u_bs = 0, v_bs = 0;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;      // Dm, chi, eta
};
struct FormJob {
    int type = FORM_NONE;
    int batch = 0;
    double* out = nullptr;
    WMassSpec w;
    LoadSpec l;
    ChtxsMatSpec c;
};
// Collects forms and launches them together; forms of one group must not depend on each other's output.
// (FEMFCT_FORM_GROUPS=0: every form in its own launch, in the order given -- the same bits.)
struct FormGroup {
    femfct_ctx* ctx;
    int n = 0;
    FormJob jobs[3];
    bool has_obs = false;       // the group's load carries a snapshot misfit: the k_forms*_obs kernels
    ObsTerm obs;
    explicit FormGroup(femfct_ctx* c) : ctx(c) {}
    void weighted_mass(const WMassSpec& sp, double* out, int32_t batch);
    void load(const LoadSpec& sp, double* out, int32_t batch);
    void load_obs(const LoadSpec& sp, const ObsTerm& t, double* out, int32_t batch);   // the group's only load: any other load is launched in a group of its own
    void chtxs_matrix(int adjoint, VecRef u, int64_t u_bs, VecRef v, int64_t v_bs, double Dm, double chi, double eta,
                      double* out, int32_t batch);
    int launch();
};

MeshArgs femfct_mesh_args(const femfct_ctx* ctx);
int femfct_enqueue_weighted_mass(femfct_ctx* ctx, const WMassSpec& sp, double* out, int32_t batch);
int femfct_enqueue_load(femfct_ctx* ctx, const LoadSpec& sp, double* out, int32_t batch);
int femfct_enqueue_react_load(femfct_ctx* ctx, const ReactLoadSpec& sp, double* out, int32_t batch);
int femfct_enqueue_obs_load(femfct_ctx* ctx, const ObsLoadSpec& sp, double* out, int32_t batch);
int femfct_enqueue_obs_terminal(femfct_ctx* ctx, double tau, const double* window, const double* uhat, int64_t uhat_bs,
                                const double* u, int64_t u_bs, double* p, int64_t p_bs, int32_t batch);
// the snapshot load minus the penalty term of the state bounds, one launch; the terminal condition with its penalty part,
// p_Nt = tau ws_obs (uhat - u) - sigma[0] gamma ws .* v (sigma: a device pointer to the level's weight)
int femfct_enqueue_bound_load(femfct_ctx* ctx, const ObsLoadSpec& sp, const BoundSpec& bs, double* out, int32_t batch);
int femfct_enqueue_bound_terminal(femfct_ctx* ctx, double tau, const double* window, const double* uhat, int64_t uhat_bs,
                                  const double* u, int64_t u_bs, const double* sigma, double gamma, const double* lo,
                                  const double* hi, const double* ws, double* p, int64_t p_bs, int32_t batch);
int femfct_enqueue_chtxs_matrix(femfct_ctx* ctx, int adjoint, VecRef u, int64_t u_bs, VecRef v, int64_t v_bs,
                                double Dm, double chi, double eta, double* out, int32_t batch);
int femfct_enqueue_growth_load(femfct_ctx* ctx, const GrowthLoadSpec& sp, double* out, int32_t batch);
// the chemotaxis flux matrix of a step (c.p0, p1, p2 = Dm, chi, eta) and its growth load in one launch
int femfct_enqueue_chtxs_matrix_growth(femfct_ctx* ctx, int adjoint, const ChtxsMatSpec& c, double* mat_out,
                                       const GrowthLoadSpec& sp, double* load_out, int32_t batch);
// the same launches with a snapshot misfit in the load (k_*_obs in kernels_forms.hip, kernels_growth.hip); the forms are those of the kernels above
int femfct_enqueue_load_obs(femfct_ctx* ctx, const LoadSpec& sp, const ObsTerm& t, double* out, int32_t batch);
int femfct_enqueue_forms_obs(femfct_ctx* ctx, const FormJob* jobs, int cnt, const ObsTerm& t);
int femfct_enqueue_chtxs_matrix_growth_obs(femfct_ctx* ctx, const ChtxsMatSpec& c, double* mat_out, const GrowthLoadSpec& sp,
                                           const ObsTerm& t, double* load_out, int32_t batch);     // adjoint matrix
int femfct_enqueue_chtxs_rhs_q_obs(femfct_ctx* ctx, VecRef u, int64_t u_bs, VecRef p, int64_t p_bs, double chi, double eta,
                                   const ObsTerm& t, double* out, int32_t batch, VecRef mx, int64_t mx_bs, double s0, double s2);
// mx.base != null: out = s0 * M mx + s2 * rhs_q in the same pass (the species right-hand side, helpers.py:1538)
int femfct_enqueue_chtxs_rhs_q(femfct_ctx* ctx, VecRef u, int64_t u_bs, VecRef p, int64_t p_bs, double chi, double eta,
                               VecRef da, int64_t da_bs, VecRef db, int64_t db_bs, double* out, int32_t batch,
                               VecRef mx = VecRef{nullptr, nullptr, 0, 0}, int64_t mx_bs = 0, double s0 = 0.0, double s2 = 0.0);

// Jacobi-preconditioned BiCGStab for the non-FCT implicit solves (kernels_krylov.hip)
struct KrylovCtl {
    int32_t flags;       // 1: breakdown, FEMFCT_FLAG_SOLVER_BUDGET: budget exhausted
    int32_t iters;
    int32_t done;
    int32_t pad;
    double resid;        // ||r||_inf / ||b||_inf
    double bnorm;
    double rho2[2];      // rho of iteration it at [it & 1] (two slots: no same-kernel read/write)
    double alpha, omega;
};
// lowsolve = true: the low-order solve of the FCT step (own control blocks, tolerance rel_tol; the
// result is reported through StepCtl by femfct_enqueue_kry_to_stepctl)
int femfct_enqueue_bicgstab(femfct_ctx* ctx, const double* mat, int32_t mat_shared, const double* b, VecRef x0,
                            int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget,
                            bool lowsolve = false);
// Chebyshev variant (structured vertex-order mesh) and the per-sweep-kind choice between the two
bool femfct_species_cheb(const femfct_ctx* ctx, int kind);
bool femfct_mesh_solve_fits(const femfct_ctx* ctx);
int femfct_enqueue_cheb_solve(femfct_ctx* ctx, const double* mat, int32_t mat_shared, const double* b, VecRef x0,
                              int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget, double tau);
int femfct_enqueue_species_solve(femfct_ctx* ctx, int kind, const double* mat, int32_t mat_shared, const double* b,
                                 VecRef x0, int64_t x0_bs, VecRef x_out, int64_t out_bs, int32_t batch, int32_t budget,
                                 double tau);   // tau: dt * diffusion coefficient of the system matrix (< 0: unknown)
int femfct_enqueue_kry_to_stepctl(femfct_ctx* ctx, int g_build, int32_t batch);
