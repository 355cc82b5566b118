/*
 * femfct.h -- C ABI of libfemfct.so, the MI355X (gfx950) FEM-FCT forward/adjoint
 * time-stepping core.
 *
 * The reference (KarolinaBenkova/FEM-FCT-PDECO) has no FFI layer: its boundary
 * is the Python call signature of helpers.py.  Each entry point below names the
 * reference interface (file:line under /root/reference) it replaces; the Python
 * mirror of those signatures lives in fem-fct-pdeco_amd/ and binds this header
 * through ctypes.
 *
 * Conventions
 *   - plain C, no C++ types or exceptions cross the ABI; every function returns
 *     an int status (FEMFCT_OK = 0) unless documented otherwise;
 *   - one femfct_ctx = one GPU + one HIP stream; a ctx is not thread-safe,
 *     distinct ctxs are independent (one process per GPU);
 *   - the caller owns host buffers; device buffers are either owned by the ctx
 *     or allocated by the caller (femfct_malloc, or any hipMalloc'd pointer such
 *     as torch.Tensor.data_ptr());
 *   - all arithmetic is IEEE float64; indices are int32;
 *   - "dev" pointers are device pointers, "host" pointers are host pointers;
 *   - all work is enqueued on the ctx stream; functions taking host output
 *     buffers synchronise before returning, pure-device functions do not.
 *
 * Data layout (device)
 *   vector        double[n]                      (DoF order chosen at pattern set-up)
 *   trajectory    double[(Nt+1)*n], level k at [k*n,(k+1)*n)   (helpers.py:563-564)
 *   ELL matrix    double[W*n], slot-major: entry (row i, slot s) at [s*n+i];
 *                 slot 0 is the diagonal; unused slots have column i and value 0
 *   batch         B independent systems: vector b at [b*n], ELL b at [b*W*n],
 *                 trajectory b at [b*(Nt+1)*n]
 */
#ifndef FEMFCT_H
#define FEMFCT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEMFCT_ABI_VERSION 5   /* 5: femfct_build_id, FEMFCT_REGIME_MESH, femfct_{nonlinear,schnak,chtxs}_forward_ct, femfct_nonlinear_adjoint_alltime, femfct_linear_trial_costs, femfct_source_trials, femfct_chtxs_{forward,adjoint}_g, femfct_{nonlinear,schnak,chtxs}_adjoint_obs (added later, backward compatible); 4: femfct_patch_walkers; 3: femfct_kernel_regime, femfct_lowop_nonzero_fraction, femfct_chebsi_md, femfct_schnak_*_tw; 2: femfct_schnak_adjoint(alltime), species solver / PDECO / source-term entry points */

typedef struct femfct_ctx femfct_ctx;

/* status codes */
#define FEMFCT_OK                 0
#define FEMFCT_ERR_INVALID        1   /* bad argument / call order (ValueError in the Python mirror) */
#define FEMFCT_ERR_HIP            2   /* HIP runtime error, text in femfct_last_error */
#define FEMFCT_ERR_NOT_CONVERGED  3   /* an iterative solve missed its tolerance */
#define FEMFCT_ERR_NOMEM          4

/* femfct_step_info.flags */
#define FEMFCT_FLAG_MMATRIX_ROWSUM 1  /* some row sum of the low-order matrix <= 0:
                                         the "3: False" diagnostic of helpers.py:1796-1799 */
#define FEMFCT_FLAG_SOLVER_BUDGET  2  /* sweep/iteration budget exhausted before tolerance */
#define FEMFCT_FLAG_COARSE_ITERS   4  /* solver_iters is an upper bound (whole fused launches), not the exact count */
#define FEMFCT_FLAG_CHEBYSHEV      8  /* species solve done by the Chebyshev iteration; solver_iters is the count that
                                         meets tolerance/10 at its asymptotic rate (the next sweep's budget) */
#define FEMFCT_FLAG_ROW_PAIRS      16 /* internal to a trajectory sweep: the pair-compact Jacobi launch met a row with both
                                         entries of an opposing stencil pair; the sweep is repeated with full rows, so
                                         a caller never sees this flag after a successful call */

/* DoF numbering of the structured mesh */
#define FEMFCT_ORDER_VERTEX 0         /* iy*N+ix (dolfin vertex order) */
#define FEMFCT_ORDER_FENICS 1         /* FEniCS CG1 dof order: rank of (ix-iy, iy) */

/* low-order solver selection */
#define FEMFCT_SOLVER_JACOBI   0      /* Jacobi sweeps, device-side convergence test (default; fused multi-sweep kernels) */
#define FEMFCT_SOLVER_BICGSTAB 1      /* Jacobi-preconditioned BiCGStab: for operators far outside the scheme's
                                         dt restriction, where Jacobi would need hundreds of sweeps */

typedef struct femfct_step_info {
    int32_t flags;          /* FEMFCT_FLAG_* */
    int32_t solver_iters;   /* sweeps / iterations used by the low-order solve */
    double  solver_resid;   /* ||b - L x||_inf / ||b||_inf of the iterate before the last sweep */
    double  min_rowsum;     /* min_i sum_j L_ij (helpers.py:1796) */
} femfct_step_info;

/* ------------------------------------------------------------------ context */
int         femfct_abi_version(void);
/* 16 hex digits: sha256 over the library's source files (names + contents) as they were when THIS binary was compiled.
 * Measurement records (bench.py, profiles/traffic.json) are stamped with it.  No reference counterpart. */
const char* femfct_build_id(void);
int         femfct_create(femfct_ctx** ctx, int device_id);
int         femfct_destroy(femfct_ctx* ctx);
const char* femfct_last_error(const femfct_ctx* ctx);
int         femfct_synchronize(femfct_ctx* ctx);
void*       femfct_stream(femfct_ctx* ctx);                 /* hipStream_t */
int         femfct_set_solver(femfct_ctx* ctx, int solver, double rel_tol, int max_iters);
int         femfct_set_graphs(femfct_ctx* ctx, int enable); /* hipGraph replay of the step sequence (default on) */
/* 1 while sweeps are replayed as hipGraphs.  0 after femfct_set_graphs(0), during per-class profiling, and while a
 * rocprofiler-sdk tool (rocprofv3) is attached to the process: its HSA queue interceptor in ROCm 7.2.0 reads a graph
 * launch's packet batch past the end of the queue ring (host SIGSEGV); FEMFCT_PROFILER_GRAPHS=1 overrides.  No reference
 * counterpart (diagnostic). */
/* Which bandwidth-regime kernels the most recent step / sweep enqueued: out[0] Jacobi launch (0 none or another regime,
 * 1 one workgroup per patch, 2 k_strip4_jacobi_walk, 3 k_strip_jacobi_pair_walk), out[1] its walkers, out[2] interior patches
 * per side of the split Chebyshev launch (0: not split), out[3] halo depth.  No reference counterpart (diagnostic). */
int         femfct_launch_info(const femfct_ctx* ctx, int32_t* out4_host);
/* What the latency-regime tile launchers made of FEMFCT_TILE_TRIM: out[0] the bits in effect, out[1] / out[2] whether a launch was
 * enqueued with the owning-wave epilogue / with write-through stores, out[3] partial slots per array of the most recent deferred-test
 * solve (0: one per workgroup).  No reference counterpart (diagnostic). */
int         femfct_tile_trim_info(const femfct_ctx* ctx, int32_t* out4_host);
int         femfct_graph_replay_active(const femfct_ctx* ctx, int* active_host);
/* 1 when the most recent femfct_solidbody_forward / _adjoint evaluated the rotation operator from the node positions
 * (large meshes, operator from femfct_assemble_rotation), 0 when it loaded the stored array.  Diagnostic. */
int         femfct_rotation_derived(const femfct_ctx* ctx, int* derived_host);
/* multi-sweep fusion of the Jacobi / Chebyshev kernels: row strips (any banded pattern) and 2-D tiles
 * (structured mesh in vertex order); both default on, results agree with the one-sweep kernels to the
 * solver tolerance.  For tests and tuning. */
int         femfct_set_fusion(femfct_ctx* ctx, int strips, int tiles);
/* kernel family a step with `batch` members uses on the registered pattern (diagnostic; -1 without a pattern) */
#define FEMFCT_REGIME_ROWS    0   /* one-sweep row kernels (any ELL pattern) */
#define FEMFCT_REGIME_STRIPS  1   /* multi-sweep row strips (banded patterns) */
#define FEMFCT_REGIME_TILE32  2   /* 32 x 32-patch tiles, latency regime (structured mesh, vertex order) */
#define FEMFCT_REGIME_PATCH64 3   /* 64 x 64-patch register/DPP kernels, bandwidth regime (n * batch >= 90 000) */
#define FEMFCT_REGIME_MESH    4   /* one workgroup per trajectory, whole step in one launch (structured mesh, vertex order,
                                     N <= 42 nodes per side, from FEMFCT_MESH_STEP_BATCH trajectories per launch on) */
int         femfct_kernel_regime(const femfct_ctx* ctx, int32_t batch);
/* bandwidth regime: persistent workgroups per batch member of the Jacobi / Chebyshev launches for a solve of `sweeps`
 * sweeps (each walks over its share of the 64 x 64 patches; the Jacobi walkers carry the rows two vertically adjacent
 * patches share in LDS); 0 = one workgroup per patch (fewer than two patches per compute unit, other regimes,
 * FEMFCT_T4_WALK=0).  This is the count of the 1024-thread walkers; the pair-compact Jacobi launch of an upwind
 * operator (512-thread walkers, two per compute unit) uses up to twice as many -- femfct_launch_info reports the launch
 * that actually ran.  Diagnostic. */
int         femfct_patch_walkers(const femfct_ctx* ctx, int32_t batch, int32_t sweeps);
/* share of the off-diagonal entries of the most recent low-order operator L = M_L + dt (A - D + N) that are non-zero
 * (an upwind stencil: about one half for pure convection).  In the bandwidth regime the Jacobi launches neither store
 * nor load the vanishing ones; 1.0 when that shortcut is not in use.  Diagnostic; synchronises. */
int         femfct_lowop_nonzero_fraction(femfct_ctx* ctx, double* fraction_host);

/* Per-kernel timing with HIP events recorded on the ctx stream around every kernel of the step
 * sequence (used by bench.py for the roofline figures).  While enabled, launches are eager.
 * Classes: 0 build_low, 1 jacobi sweep, 2 dudt_rhs, 3 chebyshev step, 4 flux, 5 limit, 6 assembly, 7 other. */
int femfct_set_profiling(femfct_ctx* ctx, int enable);
int femfct_profile_report(femfct_ctx* ctx, double* total_ms_host, int32_t* launches_host, int32_t n_classes);

/* device memory helpers (so that a ctypes-only host needs no other GPU library) */
int femfct_malloc(femfct_ctx* ctx, void** dev_ptr, size_t bytes);
int femfct_free(femfct_ctx* ctx, void* dev_ptr);
int femfct_memcpy_h2d(femfct_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int femfct_memcpy_d2h(femfct_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int femfct_memcpy_d2d(femfct_ctx* ctx, void* dev_dst, const void* dev_src, size_t bytes);
int femfct_memset0(femfct_ctx* ctx, void* dev_ptr, size_t bytes);

/* ----------------------------------------------------------------- pattern
 * Replaces find_node_neighbours (helpers.py:271-307) + the implicit CSR pattern
 * of assemble_sparse (helpers.py:87-104).  The pattern must be structurally
 * symmetric and contain the diagonal. */
int femfct_set_pattern_csr(femfct_ctx* ctx, int32_t n, const int32_t* indptr_host,
                           const int32_t* indices_host);
/* RectangleMesh(Point(a1,a1),Point(a2,a2),n_cells,n_cells) + FunctionSpace(mesh,'CG',1)
 * (advection_solidbody_FCT_PDECO_finaltime.py:63-64); also assembles M, M_lumped and
 * the stiffness matrix Ad on the device (helpers.py:553-555). */
int femfct_set_mesh_square(femfct_ctx* ctx, double a1, double a2, int32_t n_cells, int32_t order);
int32_t femfct_n(const femfct_ctx* ctx);
int32_t femfct_ell_width(const femfct_ctx* ctx);
/* ELL structure back to the host (tests, INTEGRATION): cols[W*n] */
int femfct_get_ell_cols(femfct_ctx* ctx, int32_t* cols_host);

/* CSR values on the registered pattern (host) <-> ELL values (device) */
int femfct_csr_to_ell(femfct_ctx* ctx, const double* csr_vals_host, double* ell_dev);
int femfct_ell_to_csr(femfct_ctx* ctx, const double* ell_dev, double* csr_vals_host);
/* mass matrix M (CSR values on the pattern) and diag of row_lump(M) (helpers.py:309-328)
 * for a generic pattern; not needed after femfct_set_mesh_square */
int femfct_set_mass(femfct_ctx* ctx, const double* M_csr_vals_host, const double* ml_host);
/* device pointers to the ctx-owned constant operators (ELL / vector) */
const double* femfct_mass_ell(const femfct_ctx* ctx);
const double* femfct_stiffness_ell(const femfct_ctx* ctx);
const double* femfct_lumped_mass(const femfct_ctx* ctx);

/* ----------------------------------------------------------- step operator */
/* FCT_alg_ref(A, rhs, u_n, dt, nodes, M, M_lumped, dof_neighbors, non_flux_mat)
 * helpers.py:1715-1872.  All pointers are device pointers; N_ell and rhs may be
 * NULL (= zero).  batch >= 1 independent systems (see layout above); N_shared != 0
 * means one N_ell is shared by the whole batch.  Asynchronous on the ctx stream.
 * The low-order solve runs a budget of sweeps that the context adapts from femfct_last_step_info to what the previous
 * steps needed (it starts anew with every registered pattern).  A member that the budget did not suffice for carries
 * FEMFCT_FLAG_SOLVER_BUDGET there; femfct_last_step_info then raises the budget, and the step is to be repeated (as
 * femfct_fct_step_host does by itself) until the flag is gone or the budget has reached femfct_set_solver's max_iters. */
int femfct_fct_step(femfct_ctx* ctx, const double* A_ell, const double* N_ell, int32_t N_shared,
                    const double* rhs, const double* u_n, double dt, double* u_out, int32_t batch);
/* diagnostics of the most recent femfct_fct_step (synchronises) */
int femfct_last_step_info(femfct_ctx* ctx, femfct_step_info* info_host, int32_t batch);

/* host-buffer convenience form of the same call (CSR values on the pattern;
 * uploads, runs, downloads, synchronises) */
int femfct_fct_step_host(femfct_ctx* ctx, const double* A_csr_vals, const double* N_csr_vals,
                         const double* rhs, const double* u_n, double dt, double* u_out,
                         femfct_step_info* info);

/* ChebSI(vec, M, Md, cheb_iter, lmin, lmax)  helpers.py:143-185 (M = registered mass matrix,
 * Md = its diagonal). */
int femfct_chebsi(femfct_ctx* ctx, const double* b_dev, double* y_dev, int32_t cheb_iter,
                  double lmin, double lmax, int32_t batch);
/* The same with a caller-supplied preconditioner diagonal Md != diag(M) (third argument of ChebSI, helpers.py:143,
 * 181-182: z = r / (Md * (lmin+lmax)/2)); one system per call (batch must be 1), one-sweep row kernels. */
int femfct_chebsi_md(femfct_ctx* ctx, const double* b_dev, double* y_dev, const double* md_dev, int32_t cheb_iter,
                     double lmin, double lmax, int32_t batch);
/* artificial_diffusion_mat(mat)  helpers.py:206-242: D_ell from K_ell (diagonal included) */
int femfct_artificial_diffusion(femfct_ctx* ctx, const double* K_ell, double* D_ell, int32_t batch);
/* y = alpha * Mat * x + beta * y  with an ELL matrix on the registered pattern */
int femfct_spmv(femfct_ctx* ctx, const double* mat_ell, const double* x_dev, double alpha,
                double beta, double* y_dev, int32_t batch);

/* ------------------------------------------------ structured-mesh assembly
 * Device replacements of the dolfin assembly calls on the hot path (helpers.py:87-141). */

/* coordinates of the 6 quadrature points of every triangle, layout
 * [((cy*n_cells+cx)*2 + type)*6 + q], type 0 = (v0,v1,v3), 1 = (v0,v2,v3); host arrays of
 * n_cells*n_cells*2*6 doubles.  The host evaluates its wind (a dolfin Expression in the
 * reference, helpers.py:506-508, 876-878) at these points. */
int femfct_mesh_quad_points(femfct_ctx* ctx, double* xq_host, double* yq_host);
/* scale * assemble_sparse(dot(wind, grad(v))*u*dx)  (helpers.py:581,933,1015;
 * advection_solidbody_FCT_PDECO_finaltime.py:122); wind_q_host[.. *2 + {0,1}] at the points above. */
int femfct_assemble_convection(femfct_ctx* ctx, const double* wind_q_host, double scale, double* A_ell_dev);
/* The same form for the rigid rotation wind = omega * (-x[1], x[0]) (advection_solidbody_FCT_PDECO_finaltime.py:91-93,122
 * with omega = 1/om) in closed form: the wind is linear, so int_K (w.grad v) u dx = grad v . |K|/12 (w_0 + w_1 + w_2 + w_k)
 * -- the integral the quadrature above evaluates, equal to it up to rounding.  An operator assembled here is recognised
 * (bit for bit) by femfct_solidbody_forward / _adjoint, whose large-mesh step kernels then evaluate its rows from the node
 * positions instead of loading them (FEMFCT_GEOM_ROT=0: always load). */
int femfct_assemble_rotation(femfct_ctx* ctx, double omega, double* A_ell_dev);
/* rhs_dk = -(beta*M*c + assemble(p*dot(drift, grad(u))*v*dx)) for `levels` consecutive time levels
 * (advection_solidbody_FCT_PDECO_finaltime.py:228-236); feed to femfct_chebsi(batch=levels). */
int femfct_drift_gradient_rhs(femfct_ctx* ctx, const double* c_dev, const double* u_dev, const double* p_dev,
                              double beta, double bx, double by, double* out_dev, int32_t levels);

/* ------------------------------------------------------ trajectory sweeps
 * Device-resident time loops.  Trajectories are (num_steps+1)*n doubles, level-major;
 * batch member b of a trajectory argument starts at b*(num_steps+1)*n.  c_shared != 0: one
 * control trajectory for the whole batch.  Each call synchronises once at its end (it reads
 * the per-step solver log) and returns FEMFCT_ERR_NOT_CONVERGED if a low-order solve missed
 * the tolerance even with max_iters sweeps. */

/* state sweep of the drift-control problem, u level 0 = initial condition (in place):
 * advection_solidbody_FCT_PDECO_finaltime.py:175-193  (A_u = -eps*Ad + rot_scale*Arot + Adrift1 + Adrift2,
 * control at level n+1, FCT_alg(A_u,...) == FCT_alg_ref(-A_u,...)) */
int femfct_solidbody_forward(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                             double* u_traj, int32_t num_steps, double dt, double eps, double rot_scale,
                             double bx, double by, int32_t batch);
/* the same sweep with a source term: rhs_{n+1} = assemble(src_{n+1}*v*dx) with src a trajectory, e.g. g + c of the
 * linear source-control problems (advection_FCT_PDECO_alltime_exact.py:249-253, A_u = A - eps*Ad: pass the
 * convection matrix as Arot_ell, rot_scale = 1 and a zero control).  src_traj NULL: no source. */
int femfct_solidbody_forward_src(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                 const double* src_traj, double* u_traj, int32_t num_steps, double dt, double eps,
                                 double rot_scale, double bx, double by, int32_t batch);
/* adjoint sweep: advection_solidbody_FCT_PDECO_finaltime.py:200-221 (alltime = 0: uhat is n doubles
 * per batch member, p(T) = uhat - u(T), zero rhs) and advection_solidbody_FCT_PDECO_alltime.py:232-259
 * (alltime = 1: uhat is a trajectory, p(T) = 0, rhs = assemble((uhat_n - u_n)*v*dx)) */
int femfct_solidbody_adjoint(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                             const double* u_traj, const double* uhat, double* p_traj, int32_t num_steps,
                             double dt, double eps, double rot_scale, double bx, double by, int32_t alltime,
                             int32_t batch);
/* Linear advection-diffusion-reaction with an explicit (IMEX) reaction term, du/dt - eps*lap(u) + div(w u) + g u = src
 * (advection_FCT_PDECO_finaltime_exact.py; added after ABI version 5, backward compatible).  g_traj: nodal values of the
 * P1 coefficient at every level, one trajectory shared by the batch.
 * State / sensitivity sweep, :252-279 and :344-370: rhs_{n+1} = assemble(src_{n+1}*v*dx) - Mg(g_n) u_n with
 * Mg(g) = assemble(g_h*u*v*dx), then FCT_alg(A - eps*Ad, ...); A_ell = assemble(dot(w, grad(v))*u*dx).  src_traj NULL: no
 * source.  u level 0 = initial condition (in place). */
int femfct_linear_forward_react(femfct_ctx* ctx, const double* A_ell, const double* src_traj, const double* g_traj,
                                double* u_traj, int32_t num_steps, double dt, double eps, int32_t batch);
/* Adjoint sweep, :293-322: rhs_n = -Mg(g_n) p_{n+1} (alltime != 0: + assemble((uhat_n - u_n)*v*dx)), then
 * FCT_alg(-Aadj - eps*Ad, ...) with Aadj_ell = Aa1 + Aa2, Aa2 = assemble(sigma_h*u*v*dx) for a nodal sigma ~ div(w).
 * Terminal condition and uhat as in femfct_solidbody_adjoint. */
int femfct_linear_adjoint_react(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                const double* uhat, double* p_traj, int32_t num_steps, double dt, double eps,
                                int32_t alltime, int32_t batch);
/* the load of one level on its own: out = M src - Mg(g) x, matrix-free; g is n doubles shared by the batch, src (may be
 * NULL: no M src term), x and out are n doubles per batch member */
int femfct_react_load(femfct_ctx* ctx, const double* src_dev, const double* g_dev, const double* x_dev, double* out_dev,
                      int32_t batch);
/* Tracking the state at chosen time levels (snapshot observations; added after ABI version 5, backward compatible):
 *   J = 1/2 sum_n w_n (u_n - uhat_n)^T Mw (u_n - uhat_n),  Mw = assemble(omega_h*u*v*dx), = M without a window.
 * The adjoint sweep ends in p_Nt = tau * omega .* (uhat_Nt - u_Nt) (nodal; not read if tau == 0) and loads the step to
 * level n with (theta[n]/dt) Mw (uhat_n - u_n).  uhat_traj: (num_steps + 1)*n doubles per batch member, read at the levels
 * of non-zero weight only.  theta: num_steps + 1 doubles ON THE DEVICE, owned by the caller (theta[num_steps] unused: tau
 * is that level's weight).  window: n doubles on the device, omega >= 0 in the problem's DoF order, or NULL (omega = 1).
 * (tau, theta) = (1, 0) and (0, dt) are femfct_solidbody_adjoint with alltime = 0 and 1, bit for bit. */
int femfct_solidbody_adjoint_obs(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                 const double* u_traj, const double* uhat_traj, const double* theta, double tau,
                                 const double* window, double* p_traj, int32_t num_steps, double dt, double eps,
                                 double rot_scale, double bx, double by, int32_t batch);
/* the same for the sweep with the explicit reaction term: rhs_n = (theta[n]/dt) Mw (uhat_n - u_n) - Mg(g_n) p_{n+1} */
int femfct_linear_adjoint_react_obs(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                    const double* uhat_traj, const double* theta, double tau, const double* window,
                                    double* p_traj, int32_t num_steps, double dt, double eps, int32_t batch);
/* the load of one level on its own: out = (theta_dev[level]/dt) Mw (a - b); a, b, out: n doubles per batch member.
 * theta_dev[level] == 0: out = 0, a and b are not read. */
int femfct_obs_load(femfct_ctx* ctx, const double* a_dev, const double* b_dev, const double* theta_dev, int32_t level,
                    double dt, const double* window_dev, double* out_dev, int32_t batch);
/* out_host[b] = 1/2 sum_n cost_w_dev[n] (u_n - uhat_n)^T Mw (u_n - uhat_n) of batch member b (trajectories of
 * (num_steps + 1)*n doubles); cost_w_dev: num_steps + 1 doubles on the device, levels of zero weight are not read.  The
 * result of a member does not depend on the batch size.  Synchronises. */
int femfct_obs_cost(femfct_ctx* ctx, const double* u_traj, const double* uhat_traj, const double* cost_w_dev,
                    const double* window_dev, int32_t num_steps, int32_t batch, double* out_host);
/* State bounds lower <= u_n <= upper as a Moreau-Yosida penalty on top of the snapshot tracking (added after ABI version 5,
 * backward compatible; an extension without a counterpart in the reference):
 *   v_n = u_n - clip(u_n, lower, upper),   P = gamma/2 sum_n sigma[n] sum_i ml_i window_s_i v_{n,i}^2,   J_gamma = J + P
 * with the lumped mass ml of the context's mesh.  The adjoint sweep ends in
 * p_Nt = tau * omega .* (uhat_Nt - u_Nt) - sigma[num_steps] gamma window_s .* v_Nt and loads the step to level n with
 * (theta[n]/dt) Mw (uhat_n - u_n) - (sigma[n]/dt) gamma ml .* window_s .* v_n in the one load launch of the step.
 * lower, upper: n doubles on the device in the problem's DoF order (+-inf allowed), either may be NULL (no bound on that
 * side), not both.  sigma: num_steps + 1 level weights >= 0 ON THE DEVICE (sigma[0] = 0 for a fixed initial condition; a
 * level of zero weight is not read for the penalty, the last level included, and no level is with gamma = 0).  window_s: n doubles >= 0 on the device, or NULL (1).  gamma: finite,
 * >= 0.  Without a violation the results are those of the _obs entry points, bit for bit.  A NaN in a penalised u_n gives
 * a NaN load (the sweep fails as it does for a NaN state). */
int femfct_solidbody_adjoint_bounds(femfct_ctx* ctx, const double* Arot_ell, const double* c_traj, int32_t c_shared,
                                    const double* u_traj, const double* uhat_traj, const double* theta, double tau,
                                    const double* window, const double* lower, const double* upper, double gamma,
                                    const double* sigma, const double* window_s, double* p_traj, int32_t num_steps,
                                    double dt, double eps, double rot_scale, double bx, double by, int32_t batch);
int femfct_linear_adjoint_react_bounds(femfct_ctx* ctx, const double* Aadj_ell, const double* g_traj, const double* u_traj,
                                       const double* uhat_traj, const double* theta, double tau, const double* window,
                                       const double* lower, const double* upper, double gamma, const double* sigma,
                                       const double* window_s, double* p_traj, int32_t num_steps, double dt, double eps,
                                       int32_t batch);
/* the load of one level on its own: out = (theta_dev[level]/dt) Mw (uhat - u) [- Mg(g) x]
 * - (sigma_dev[level]/dt) gamma ml .* window_s .* v(u); uhat, u, x, out: n doubles per batch member, g (with x; both
 * NULL: no reaction part) shared by the batch.  theta_dev[level] == 0: uhat is not read. */
int femfct_bound_load(femfct_ctx* ctx, const double* uhat_dev, const double* u_dev, const double* theta_dev,
                      const double* sigma_dev, int32_t level, double dt, const double* window_dev, const double* g_dev,
                      const double* x_dev, const double* lower_dev, const double* upper_dev, double gamma,
                      const double* window_s_dev, double* out_dev, int32_t batch);
/* out_host[3 b + {0, 1, 2}] = P, the largest |v| and the number of v != 0 (as a double) of batch member b over the
 * penalised (level, node) pairs, those with sigma_dev[n] != 0 and window_s_i != 0 (trajectories of (num_steps + 1)*n
 * doubles).  The result of a member does not depend on the batch size.  Synchronises. */
int femfct_bound_cost(femfct_ctx* ctx, const double* u_traj, const double* sigma_dev, const double* lower_dev,
                      const double* upper_dev, double gamma, const double* window_s_dev, int32_t num_steps, int32_t batch,
                      double* out_host);
/* out_ell = assemble(f_h*u*v*dx) for the P1 function with nodal values f_dev (n doubles).  Synchronises. */
int femfct_assemble_weighted_mass(femfct_ctx* ctx, const double* f_dev, double* out_ell);
/* solver diagnostics of the most recent sweep: info_host[step*batch + b] */
int femfct_traj_info(femfct_ctx* ctx, femfct_step_info* info_host, int32_t num_steps, int32_t batch);

/* ------------------------------------------------------ optimisation layer
 * Reductions/updates of the projected-gradient loop kept on the device (only scalars
 * cross PCIe).  M is the registered mass matrix; results are written to host memory
 * (these calls synchronise).  batch member b of a trajectory starts at b*(num_steps+1)*n. */

/* L2_norm_sq_Q(phi, num_steps, dt, M)  helpers.py:330-360, phi = a - b (b may be NULL) */
int femfct_l2_norm_sq_Q(femfct_ctx* ctx, const double* a_dev, const double* b_dev, int32_t num_steps,
                        double dt, double* out_host, int32_t batch);
/* L2_norm_sq_Omega(phi, M)  helpers.py:362-381, phi = a - b, one level of n doubles per batch member */
int femfct_l2_norm_sq_Omega(femfct_ctx* ctx, const double* a_dev, const double* b_dev, double* out_host,
                            int32_t batch);
/* cost_functional(var1, var1_target, projected_control, num_steps, dt, M, beta, optim, var2, var2_target)
 * helpers.py:383-441; finaltime = 0: optim == "alltime" (targets are trajectories),
 * finaltime = 1: optim == "finaltime" (targets are n doubles per batch member). */
int femfct_cost_functional(femfct_ctx* ctx, const double* var1, const double* var1_target,
                           const double* control, int32_t control_shared, int32_t num_steps, double dt,
                           double beta, int32_t finaltime, const double* var2, const double* var2_target,
                           double* J_host, int32_t batch);
/* update_control: out = clip(c + s*d, c_lower, c_upper)  helpers.py:1666-1667 (out may alias c) */
int femfct_project_control(femfct_ctx* ctx, const double* c_dev, double s, const double* d_dev,
                           double c_lower, double c_upper, double* out_dev, int64_t count);

/* Armijo trial batches of the linear source-control PDECO (advection_FCT_PDECO_{alltime_exact,finaltime}.py, helpers.py:
 * 1681-1708): trial t < K has s_t = s0 * (1 / 2^t) and c_t = clip(c + s_t d, c_lower, c_upper). */
#define FEMFCT_MAX_TRIALS 16
/* Linear increment: J_host[t] = cost_functional(u + s_t w, uhat, c_t, ...) and dist_host[t] = L2_norm_sq_Q(c_t - c), all K
 * trials in one pass over the five trajectories (one trajectory each, (num_steps+1)*n doubles; uhat is n doubles when
 * finaltime).  Bitwise equal to materialising each trial (femfct_project_control, femfct_axpby(1, u, s_t, w)) and calling
 * femfct_cost_functional and femfct_l2_norm_sq_Q.  Synchronises. */
int femfct_linear_trial_costs(femfct_ctx* ctx, const double* u_dev, const double* w_dev, const double* uhat_dev,
                              const double* c_dev, const double* d_dev, double s0, int32_t K, double c_lower,
                              double c_upper, double beta, int32_t num_steps, double dt, int32_t finaltime,
                              double* J_host, double* dist_host);
/* Resolve mode: c_out[t*count ..] = c_t and src_out[t*count ..] = g + c_t (g NULL: c_t; src_out may be NULL), the
 * expressions of femfct_project_control and femfct_axpby(1, g, 1, c_t), in one launch. */
int femfct_source_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0,
                         int32_t K, double c_lower, double c_upper, int64_t count, double* c_out_dev,
                         double* src_out_dev);

/* Lockstep batches of the drift-control PGD (config C5's regularisation sweep as one loop): P problems, each with K
 * Armijo trials, advance together; member m = p*K + t stands for problem p < P and trial t < K, 1 <= P*K <= 256. */
#define FEMFCT_MAX_MEMBERS 256
/* c_out[m*count + k] = clip(c[p*count + k] + steps_host[p*K + t] * d[p*count + k], c_lower, c_upper): bitwise what P*K
 * calls of femfct_project_control write (c, d: P blocks of count doubles; c_out: P*K; must not alias them).  The steps
 * are read before the call returns.  One launch, does not synchronise. */
int femfct_trial_controls(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* steps_host, int32_t P,
                          int32_t K, double c_lower, double c_upper, int64_t count, double* c_out_dev);
/* J_host[m] = cost_functional(u_m, uhat_p, c_m, ..., beta_host[p], finaltime) and dist_host[m] = L2_norm_sq_Q(c_m - cref_p)
 * for the P*K member trajectories u_traj / c_traj ((num_steps+1)*n doubles each), bitwise what femfct_cost_functional and
 * femfct_l2_norm_sq_Q return for each member alone, in one fused pass; levels * members is not limited.  uhat: one target
 * (uhat_per_problem = 0) or P (1), each n doubles when finaltime, else a trajectory.  cref: P reference controls, or NULL
 * (no distances; dist_host may be NULL).  Synchronises. */
int femfct_member_costs(femfct_ctx* ctx, const double* u_traj, const double* uhat, int32_t uhat_per_problem,
                        const double* c_traj, const double* cref, const double* beta_host, int32_t P, int32_t K,
                        int32_t num_steps, double dt, int32_t finaltime, double* J_host, double* dist_host);

/* Controls that are piecewise constant in time: K intervals of time levels, interval k = the levels
 * starts_host[k] <= l < starts_host[k+1] (K + 1 strictly increasing values, starts_host[0] = 0, starts_host[K] =
 * num_steps + 1; anything else is FEMFCT_ERR_INVALID).  With the trapezoid's level weights w_l of L2_norm_sq_Q (1, and
 * 1/2 at levels 0 and num_steps) and W_k = sum_{l in k} w_l,
 *   restrict:  out_dev[(b*K + k)*n + i] = (sum_{l in k} w_l x_traj[(b*(num_steps+1) + l)*n + i]) / W_k
 *   prolong:   out_traj[(b*(num_steps+1) + l)*n + i] = y_dev[(b*K + k(l))*n + i]
 * for the batch members b < batch.  prolong(restrict(.)) is the orthogonal projection, in the inner product of
 * femfct_l2_norm_sq_Q, onto the trajectories that are constant on every interval; an interval of one level returns that
 * level exactly.  The sums run in a fixed order that depends on an interval's length alone (no atomics): the same bits
 * for every batch size, member and run.  starts_host is read before the call returns.  One launch sequence per call, does
 * not synchronise.  out_dev / out_traj must not alias the call's input; the x_traj of a restrict and the out_traj of the
 * prolong that follows may be one buffer (the projection in place). */
int femfct_time_restrict(femfct_ctx* ctx, const double* x_traj, const int32_t* starts_host, int32_t K, int32_t num_steps,
                         int32_t batch, double* out_dev);
int femfct_time_prolong(femfct_ctx* ctx, const double* y_dev, const int32_t* starts_host, int32_t K, int32_t num_steps,
                        int32_t batch, double* out_traj);

/* Primitives of the limited-memory quasi-Newton loops (solvers.LimitedMemory; an extension, no reference call): a
 * direction of any memory is one call of each, and the two-loop recursion runs on the host on coefficient vectors. */
/* The free set of a box-constrained control c with gradient g, one byte per value: mask[k] = 0 (bound) iff
 * (c[k] <= c_lower && g[k] > 0) || (c[k] >= c_upper && g[k] < 0), else 1 (free).  One launch, does not synchronise. */
int femfct_free_set(femfct_ctx* ctx, const double* c_dev, const double* g_dev, double c_lower, double c_upper, int64_t count,
                    uint8_t* mask_dev);
/* The L2(Q) Gram matrix of J trajectories ((num_steps+1)*n doubles each; fields_host: J device pointers, read before the
 * call returns; the same pointer may appear twice), 1 <= J <= FEMFCT_MAX_GRAM_FIELDS:
 *   G_host[i*J + j] = dt * sum_l w_l (chi.f_i)_l^T M (chi.f_j)_l
 * with the registered mass matrix, the trapezoid weights w_l of femfct_l2_norm_sq_Q and chi = mask_dev (one byte per
 * value as femfct_free_set writes it; NULL: all free).  Entries i <= j are formed as f_i . (M f_j) and mirrored: G is
 * exactly symmetric.  The sums run in the fixed tree of femfct_l2_norm_sq_Q (no atomics): two calls return the same
 * bits, and without a mask G[i][i] = femfct_l2_norm_sq_Q(f_i) bit for bit.  Synchronises. */
#define FEMFCT_MAX_GRAM_FIELDS 17
int femfct_q_gram(femfct_ctx* ctx, const double* const* fields_host, int32_t J, const uint8_t* mask_dev, int32_t num_steps,
                  double dt, double* G_host);
/* out[k] = ((coef_0*f_0[k] + coef_1*f_1[k]) + ...) + coef_{J-1}*f_{J-1}[k] where mask[k] != 0 (the sum in index order, no
 * contraction: bitwise the NumPy expression) and fallback_scale*fallback[k] elsewhere.  mask_dev NULL: all free, and only
 * then may fallback_dev be NULL.  fields_host and coef_host (J values each) are read before the call returns.  out must
 * not alias an input.  One launch, does not synchronise. */
int femfct_q_combine(femfct_ctx* ctx, const double* const* fields_host, const double* coef_host, int32_t J,
                     const uint8_t* mask_dev, const double* fallback_dev, double fallback_scale, int64_t count,
                     double* out_dev);

/* Primitives of the proximal-gradient loops for L1-sparse controls (solvers.prox_solidbody, solvers.prox_source_control;
 * an extension, no reference call).  The cost gains alpha * ||c||_{1,h} with the nodal-quadrature norm
 *   ||c||_{1,h} = dt * sum_l w_l sum_i ml_i |c_{l,i}|
 * (w_l the trapezoid weights of femfct_l2_norm_sq_Q, ml the registered lumped mass), whose prox is pointwise. */
/* The K trial controls of a proximal step, t < K, s_t = s0 * (1 / 2^t):
 *   x = c + s_t*d, tau = s_t*alpha, v = |x| - tau > 0 ? copysign(|x| - tau, x) : 0.0, c_out[t*count + k] = fmin(fmax(v, c_lower), c_upper)
 * evaluated in this order without contraction (the exact prox of tau|.| + the box indicator, value by value), and
 * src_out[t*count ..] = g + c_t as femfct_source_trials writes it (g NULL: c_t; src_out may be NULL).  alpha = 0 gives
 * femfct_source_trials' values.  alpha < 0, K outside 1..FEMFCT_MAX_TRIALS, count <= 0 or c_lower > c_upper is
 * FEMFCT_ERR_INVALID.  c_out / src_out must not alias an input.  One launch, does not synchronise. */
int femfct_prox_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0, int32_t K,
                       double alpha, double c_lower, double c_upper, int64_t count, double* c_out_dev, double* src_out_dev);
/* out_host[b] = ||a_b||_{1,h} for the batch trajectories a ((num_steps+1)*n doubles each).  The sums run in the fixed
 * tree of femfct_l2_norm_sq_Q (no atomics): two calls return the same bits; levels * batch is not limited.  Synchronises. */
int femfct_l1_norm_Q(femfct_ctx* ctx, const double* a_dev, int32_t num_steps, double dt, double* out_host, int32_t batch);
/* For the K trial controls c_trials_dev (K trajectories, as femfct_prox_trials writes them) and the one control c_ref_dev
 * they started from, in one fused pass: l1_host[t] = femfct_l1_norm_Q(c_t) and dist_host[t] = femfct_l2_norm_sq_Q(c_t -
 * c_ref), both bit for bit, and nnz_host[t] = the number of values of c_t that are != 0.  Synchronises. */
int femfct_sparse_trial_stats(femfct_ctx* ctx, const double* c_trials_dev, const double* c_ref_dev, int32_t K,
                              int32_t num_steps, double dt, double* l1_host, double* dist_host, int64_t* nnz_host);
/* The K trial controls of a proximal step under a control budget ||c||_{1,h} <= budget (solvers.prox_solidbody and
 * prox_source_control with budget=; added after ABI version 5, backward compatible).  For t < K, s_t = s0 * (1 / 2^t),
 * tau_t = s_t*alpha, x_t = c + s_t*d:
 *   c_out[t] = clip(soft_threshold(x_t, tau_t + lambda_t), c_lower, c_upper)      (femfct_prox_trials' expression)
 * with lambda_t = 0.0 exactly, and femfct_prox_trials' bits, where that trial's norm is <= budget, else lambda_t > 0 the
 * root of ||c_out[t]||_{1,h} = budget: value by value the projection of the prox onto {box, ||.||_{1,h} <= budget} in the
 * nodal inner product with the weights dt*w_l*ml_i.  src_out[t] = 1.0*g + 1.0*c_out[t] (g NULL: c_out[t]; src_out may be
 * NULL).  d_dev NULL, with K = 1 only: x = c, tau = 0, the projection of c itself.  lambda_host[t], l1_host[t] =
 * femfct_l1_norm_Q of the written trial bit for bit, rounds_host[t] = search rounds used (<= 16; one launch and one
 * read-back of 19 K doubles each).  No atomics, fixed trees: two calls return the same bits.  budget not finite-positive,
 * alpha < 0, a box without 0, K outside 1..FEMFCT_MAX_TRIALS, num_steps < 0, no mass matrix, or a NaN / Inf in c or d
 * (found in the first read-back, before any search) is FEMFCT_ERR_INVALID.  Synchronises. */
int femfct_budget_trials(femfct_ctx* ctx, const double* c_dev, const double* d_dev, const double* g_dev, double s0, int32_t K,
                         double alpha, double budget, double c_lower, double c_upper, int32_t num_steps, double dt,
                         double* c_out_dev, double* src_out_dev, double* lambda_host, double* l1_host, int32_t* rounds_host);

/* Ensemble drift control (solvers.ensemble_solidbody; added after ABI version 5, backward compatible; an extension without
 * a counterpart in the reference): one control c serves S scenarios, 1 <= S <= FEMFCT_MAX_MEMBERS, each with its own state
 * u_s, FCT adjoint p_s, target uhat_s and weight pi_s >= 0,
 *   J(c) = sum_s pi_s T_s + beta/2 ||c||^2_Q,     T_s = femfct_obs_cost of scenario s.
 * The limiter is nonlinear, so the weights enter where the gradient is formed and not in the adjoint loads.  weights_host:
 * S values, read before the call returns; a negative or non-finite weight, or all weights zero, is FEMFCT_ERR_INVALID. */
/* out_l = -(beta M c_l + acc_l) for every level l < levels, acc = pi_s0 g_s0 for the first scenario of non-zero weight, then
 * acc = acc + pi_s g_s in index order (no contraction), g_s = assemble(p_s (b.grad u_s) v dx) row by row the expression of
 * femfct_drift_gradient_rhs.  c_dev, out_dev: one trajectory of levels*n doubles; u_traj, p_traj: S of them, scenario s at
 * s*levels*n.  A scenario of weight 0 is not read.  S = 1 with weight 1, and two equal scenarios with weights 1/2, give
 * femfct_drift_gradient_rhs's bits.  One launch with that call's geometry, does not synchronise. */
int femfct_ensemble_drift_gradient_rhs(femfct_ctx* ctx, const double* c_dev, const double* u_traj, const double* p_traj,
                                       const double* weights_host, int32_t S, double beta, double bx, double by,
                                       double* out_dev, int32_t levels);
/* T_host[s] = femfct_obs_cost of scenario s (every s, weight 0 included: diagnostics), J_host[0] = (sum_s pi_s T_s, index
 * order, non-zero weights, no contraction) + (0.5*beta) * femfct_l2_norm_sq_Q(c), dist_host[0] = femfct_l2_norm_sq_Q(c -
 * cref), each of the three bit for bit those calls' values and independent of S.  u_traj, uhat_traj: S trajectories of
 * (num_steps+1)*n doubles; cost_w_dev, window_dev: as femfct_obs_cost; c_dev, cref_dev: one trajectory each, the control
 * is read once; cref_dev and dist_host are given together or both NULL.  One pass over the scenarios, one over the
 * control, one read-back.  Synchronises. */
int femfct_ensemble_costs(femfct_ctx* ctx, const double* u_traj, const double* uhat_traj, const double* cost_w_dev,
                          const double* window_dev, const double* c_dev, const double* cref_dev,
                          const double* weights_host, int32_t S, double beta, int32_t num_steps, double dt,
                          double* T_host, double* J_host, double* dist_host);

/* Smooth controls (solvers.Smoothness; added after ABI version 5, backward compatible; an extension without a counterpart
 * in the reference): the H1 seminorm of a control trajectory c = (c_0 .. c_Nt) in space and time,
 *   R(c) = beta_x/2 R_x + beta_t/2 R_t,    R_x = dt sum_{l=0..Nt} w_l c_l^T Ad c_l,
 *                                          R_t = (1/dt) sum_{l<Nt} (c_{l+1} - c_l)^T M (c_{l+1} - c_l),
 * w the trapezoid's level weights (1/2 at the end levels), Ad = femfct_stiffness_ell, M the mass of femfct_l2_norm_sq_Q.
 * Its gradient g in that call's inner product (dR(c)[v] = dt sum_l w_l g_l^T M v_l) satisfies
 *   M g_l = beta_x Ad c_l + beta_t M tau_l,   tau_l = (2 c_l - c_{l-1} - c_{l+1})/dt^2 for 0 < l < Nt,
 *   tau_0 = 2 (c_0 - c_1)/dt^2,  tau_Nt = 2 (c_Nt - c_{Nt-1})/dt^2.
 * All three need the structured mesh (femfct_set_mesh_square), num_steps >= 1, dt > 0 and finite coefficients >= 0
 * (FEMFCT_ERR_INVALID otherwise); no atomics, fixed summation trees: two calls return the same bits. */
/* out_host[2 b] = R_x, out_host[2 b + 1] = R_t of batch member b (not scaled by the coefficients); c_dev: batch
 * trajectories of (num_steps+1)*n doubles.  One pass over c, two level folds, one read-back; levels * batch is not limited.
 * Synchronises. */
int femfct_smooth_cost(femfct_ctx* ctx, const double* c_dev, int32_t num_steps, double dt, double* out_host, int32_t batch);
/* out_l = -(beta_x (Ad c_l) + beta_t (M tau_l)) for every level and batch member, the right-hand side of the mass solve
 * that gives -g.  beta_t == 0: no neighbouring level is read; beta_x == 0: Ad is not read.  out_dev must not alias c_dev.
 * One launch, does not synchronise. */
int femfct_smooth_rhs(femfct_ctx* ctx, const double* c_dev, double beta_x, double beta_t, int32_t num_steps, double dt,
                      double* out_dev, int32_t batch);
/* out_l = femfct_drift_gradient_rhs(c, u, p, beta, bx, by)_l + femfct_smooth_rhs(c, beta_x, beta_t)_l in one launch, bit for
 * bit the sum femfct_axpby(1, ., 1, .) forms of the two; beta_x == beta_t == 0: femfct_drift_gradient_rhs's bits.
 * levels = num_steps + 1 >= 2; one trajectory each.  Does not synchronise. */
int femfct_drift_gradient_rhs_smooth(femfct_ctx* ctx, const double* c_dev, const double* u_dev, const double* p_dev,
                                     double beta, double beta_x, double beta_t, double dt, double* out_dev, int32_t levels,
                                     double bx, double by);

/* Initial-state recovery (solvers.initial_state_solidbody; added after ABI version 5, backward compatible; an extension
 * without a counterpart in the reference): the control is fixed and the initial state v = u_0 is the unknown,
 *   J(v) = T(u(v)) + beta0/2 (v - v_b)^T M (v - v_b),    g = beta0 (v - v_b) - p_0,
 * T the tracking term of femfct_cost_functional (beta = 0) / femfct_obs_cost, p the adjoint sweep of u(v) and g the
 * L2(Omega) representative of the gradient (p(T) = uhat - u(T): no mass solve).  Every field is one level of n doubles.
 * An argument error is FEMFCT_ERR_INVALID and leaves the context usable. */
/* u_traj[k*(num_steps+1)*n + i] = fmin(fmax(v[i] + steps_host[k]*dir[i], v_lower), v_upper) for the members k < K,
 * 1 <= K <= FEMFCT_MAX_MEMBERS: the trial states written into level 0 of a batch of K trajectories, where the forward
 * sweep reads them; no other level is touched.  No contraction: bitwise the NumPy expression.  The steps are read before
 * the call returns.  v_lower > v_upper is an error.  One launch, does not synchronise. */
int femfct_initial_trials(femfct_ctx* ctx, const double* v_dev, const double* dir_dev, const double* steps_host, int32_t K,
                          double v_lower, double v_upper, double* u_traj_dev, int32_t num_steps);
/* out_host[2 k] = ||v_k - v_b||^2_M and out_host[2 k + 1] = ||v_k - v||^2_M for v_k = level 0 of member k < K of the batch
 * u_traj_dev, each bit for bit femfct_l2_norm_sq_Omega(v_k, v_b) / (v_k, v) (vb_dev NULL: a zero background, that call's
 * NULL).  One pass over the members, one fold, one read-back; fixed-order sums, no atomics: two calls return the same bits,
 * and member k's entries depend on member k alone.  Synchronises. */
int femfct_initial_trial_stats(femfct_ctx* ctx, const double* u_traj_dev, const double* v_dev, const double* vb_dev,
                               int32_t K, int32_t num_steps, double* out_host);
/* g[i] = beta0*(v[i] - vb[i]) - p_traj[i] (vb_dev NULL: v[i] - 0.0), reading level 0 of the adjoint trajectory only; no
 * contraction: bitwise the NumPy expression, and beta0 = 0 gives -p_0.  mask_dev != NULL: the free set of
 * femfct_free_set(v, g, v_lower, v_upper, n) from the same pass, byte for byte (mask_dev NULL: the bounds are not used).
 * beta0 negative or non-finite is an error.  One launch, does not synchronise. */
int femfct_initial_gradient(femfct_ctx* ctx, const double* p_traj_dev, const double* v_dev, const double* vb_dev,
                            double beta0, double* g_dev, double v_lower, double v_upper, uint8_t* mask_dev);
/* The L2(Omega) Gram matrix of J one-level fields (fields_host: J device pointers, read before the call returns; the same
 * pointer may appear twice), 1 <= J <= FEMFCT_MAX_GRAM_FIELDS: G_host[i*J + j] = (chi.f_i)^T M (chi.f_j), chi = mask_dev
 * (n bytes as femfct_free_set writes them; NULL: all free; a masked-out value is not read).  The one-level sibling of
 * femfct_q_gram, whose trapezoid weights are not defined for one level.  Entries i <= j are formed as f_i . (M f_j) and
 * mirrored: exactly symmetric.  Fixed-order sums, no atomics: two calls return the same bits, and without a mask
 * G[i][i] = femfct_l2_norm_sq_Omega(f_i, NULL) bit for bit.  femfct_q_combine with count = n forms the combination.
 * Synchronises. */
int femfct_omega_gram(femfct_ctx* ctx, const double* const* fields_host, int32_t J, const uint8_t* mask_dev,
                      double* G_host);

/* Control zones: controls that are piecewise constant in space on sets of nodes (solvers.ControlZones; an extension, no
 * reference call).  labels_host: n values in the pattern's row order, -1 = no control acts at the node, 0 .. m-1 = its
 * zone; every zone is non-empty and 1 <= m <= FEMFCT_MAX_ZONES.  With chi_j the nodal indicator of zone j,
 *   restrict:  out_dev[f*m + j] = sum_{i in zone j} y_i,   y = x_f (apply_mass = 0) or y = M x_f (apply_mass = 1): chi^T (M) x
 *   prolong:   out_dev[f*n + i] = delta_f[label_i] (0.0 where label_i = -1),   delta_f = Ginv s_f (Ginv_dev NULL: s_f)
 * for the `fields` one-level fields of n values that lie back to back in x_dev / out_dev.  With G = chi^T M chi (the
 * restriction with apply_mass = 1 of the m indicator fields) and Ginv its inverse, prolong(restrict(x, 1)) is the
 * orthogonal projection in the mass inner product onto span{chi_j}, and prolong(restrict(r, 0)) the steepest-descent
 * direction among zone-constant controls for a dual right-hand side r.
 * femfct_set_control_zones registers the table (after the pattern; a new pattern drops it): a label outside -1 .. m-1, an
 * empty zone or m out of range is FEMFCT_ERR_INVALID and the previous table stays in place; labels_host NULL clears (m is
 * ignored).  It is the only call that reads labels_host, and it synchronises.
 * A row of M x is formed as the quadratic forms form it (diagonal slot, then slots 1 .. W-1); a zone's sum runs over its
 * node list (ascending) in chunks of a fixed size, chunk sums folded in order: the order depends on the zone table alone
 * (no atomics), the same bits for every `fields`, every position of a field and every run.  delta_f[j] =
 * ((Ginv[j][0] s[0] + Ginv[j][1] s[1]) + ...) in index order without contraction, Ginv_dev m x m row-major; all nodes of a
 * zone receive the same stored value.  The out_dev of a prolong may be the x_dev its restrict read.  At most two launches
 * per call, neither synchronises; without a registered table both are FEMFCT_ERR_INVALID. */
#define FEMFCT_MAX_ZONES 256
int femfct_set_control_zones(femfct_ctx* ctx, const int32_t* labels_host, int32_t m);
int femfct_zone_restrict(femfct_ctx* ctx, const double* x_dev, int64_t fields, int32_t apply_mass, double* out_dev);
int femfct_zone_prolong(femfct_ctx* ctx, const double* s_dev, const double* Ginv_dev, int64_t fields, double* out_dev);

/* descent direction of the pointwise-gradient problems, d = -(beta*c - t) with t = x*y/divisor (y given)
 * or t = scale*x (y NULL): nonlinear_FCT_PDECO_refactored.py:148, Schnak_FCT_PDECO_refactored.py:167,
 * chemotaxis_FCT_PDECO_AT_refactored.py:158 (same floating-point operation order) */
int femfct_descent_pointwise(femfct_ctx* ctx, int64_t count, double beta, const double* c_dev, double scale,
                             const double* x_dev, const double* y_dev, double divisor, double* out_dev);

/* ------------------------------------------------ non-FCT species and the three PDE systems */

/* out = in^T on the registered pattern: assemble_sparse(dot(wind,grad(u))*w*dx) (helpers.py:681) is the
 * transpose of assemble_sparse(dot(wind,grad(w))*u*dx) (helpers.py:581) */
int femfct_ell_transpose(femfct_ctx* ctx, const double* in_ell, double* out_ell);
/* out = alpha*a + beta*b over count doubles (b may be NULL): Du*Ad - omega1*A etc. (helpers.py:583) */
int femfct_axpby(femfct_ctx* ctx, int64_t count, double alpha, const double* a_dev, double beta,
                 const double* b_dev, double* out_dev);
/* tolerance / iteration cap of the iterative solver used for the non-FCT implicit solves */
int femfct_set_krylov(femfct_ctx* ctx, double rel_tol, int32_t max_iters);
/* solver of those solves inside the trajectory sweeps: FEMFCT_SPECIES_AUTO = tile-fused Chebyshev
 * iteration on the structured vertex-order mesh (falls back to BiCGStab when it does not contract),
 * FEMFCT_SPECIES_BICGSTAB = always BiCGStab.  Both meet the same residual tolerance. */
#define FEMFCT_SPECIES_AUTO 0
#define FEMFCT_SPECIES_BICGSTAB 1
int femfct_set_species_solver(femfct_ctx* ctx, int32_t mode);
/* spsolve(Mat, b) (helpers.py:596,686,1342,1538): Jacobi-preconditioned BiCGStab from the initial guess
 * x0; mat_shared != 0: one matrix for the whole batch.  Synchronises. */
int femfct_bicgstab(femfct_ctx* ctx, const double* mat_ell, int32_t mat_shared, const double* b_dev,
                    const double* x0_dev, double* x_dev, int32_t batch, femfct_step_info* info_host);

/* solve_nonlinear_equation (helpers.py:881-966).  Aw_ell = assemble_sparse(dot(wind,grad(v))*u*dx);
 * c_level = the control level the reference uses for the whole sweep (level 1, helpers.py:950-951; or
 * the constant control_fun), n doubles per batch member; u_traj level 0 = initial condition. */
int femfct_nonlinear_forward(femfct_ctx* ctx, const double* Aw_ell, const double* c_level, double* u_traj,
                             int32_t num_steps, double dt, double eps, int32_t batch);
/* solve_adjoint_nonlinear_equation (helpers.py:968-1038); uhat_T: n doubles per batch member */
int femfct_nonlinear_adjoint(femfct_ctx* ctx, const double* Aw_ell, const double* u_traj,
                             const double* uhat_T, double* p_traj, int32_t num_steps, double dt, double eps,
                             int32_t batch);
/* solve_schnak_system (helpers.py:511-597); par = {Du, Dv, c_b, gamma, omega1, omega2} */
int femfct_schnak_forward(femfct_ctx* ctx, const double* Aw_ell, const double* c_level, double* u_traj,
                          double* v_traj, int32_t num_steps, double dt, const double* par, double rescaling,
                          int32_t batch);
/* solve_adjoint_schnak_system (helpers.py:599-698); AwT_ell = femfct_ell_transpose(Aw_ell).
 * alltime = 0: the reference's final-time problem (uhat_T, vhat_T: n doubles per batch member).
 * alltime = 1: all-time misfit (targets are trajectories, p(T) = q(T) = 0, misfit loads in both equations as
 * in the inline loop of Schnak_FCT_PDECO_alltime.py:204-284; helpers.py has no such variant). */
int femfct_schnak_adjoint(femfct_ctx* ctx, const double* AwT_ell, const double* u_traj, const double* v_traj,
                          const double* uhat_T, const double* vhat_T, double* p_traj, double* q_traj,
                          int32_t num_steps, double dt, const double* par, int32_t alltime, int32_t batch);
/* The two Schnakenberg sweeps with a separable time-dependent wind w(x, t) = s(t) w0(x) -- the set-up of the script
 * BASELINE config 3 names, Schnak_FCT_PDECO_alltime.py:55,174-175,228-230 (rotation * sin(2 pi t), convection matrix
 * re-assembled every step; helpers.py:565-566, 664, 679 set wind.t the same way).  Aw_ell / AwT_ell are the matrices
 * of w0; wind_scale_host[k] = s(t_k), k = 0..num_steps (host array, copied).  The step to level n+1 (forward) uses
 * s(t_{n+1}); the step to level n (adjoint) uses s(t_n).  wind_scale_host == NULL: stationary wind (= the calls above). */
int femfct_schnak_forward_tw(femfct_ctx* ctx, const double* Aw_ell, const double* wind_scale_host, const double* c_level,
                             double* u_traj, double* v_traj, int32_t num_steps, double dt, const double* par,
                             double rescaling, int32_t batch);
int femfct_schnak_adjoint_tw(femfct_ctx* ctx, const double* AwT_ell, const double* wind_scale_host, const double* u_traj,
                             const double* v_traj, const double* uhat_T, const double* vhat_T, double* p_traj,
                             double* q_traj, int32_t num_steps, double dt, const double* par, int32_t alltime,
                             int32_t batch);
/* solve_chtxs_system (helpers.py:1250-1385, non-generation mode); par = {delta, Dm, Df, chi, eta} */
int femfct_chtxs_forward(femfct_ctx* ctx, const double* c_level, double* u_traj, double* v_traj,
                         int32_t num_steps, double dt, const double* par, double rescaling, int32_t batch);
/* solve_adjoint_chtxs_system (helpers.py:1387-1581); alltime = 0: optim "finaltime" (uhat/vhat n doubles
 * per member), 1: optim "alltime" (uhat/vhat trajectories; raw nodal misfits as in helpers.py:1506-1507,
 * 1533-1534; level num_steps of p/q is taken as passed) */
int femfct_chtxs_adjoint(femfct_ctx* ctx, const double* u_traj, const double* v_traj, const double* uhat,
                         const double* vhat, double* p_traj, double* q_traj, const double* c_traj,
                         int32_t num_steps, double dt, const double* par, double rescaling, int32_t alltime,
                         int32_t batch);
/* The three forward sweeps with a per-step control, as in the reference's all-time scripts
 * (nonlinear_FCT_PDECO_alltime.py:189-192, Schnak_FCT_PDECO_alltime.py:182-191,
 * chemotaxis_mimura_FCT_PGD_alltime.py:180-183): the step from level n to level n+1 reads level n+1 of c_traj
 * (level 0 is never read).  c_traj: (num_steps+1)*n doubles per batch member, batch stride (num_steps+1)*n;
 * c_shared != 0: one trajectory for the whole batch (as femfct_solidbody_forward).  Everything else as the frozen-level
 * calls above; femfct_schnak_forward_ct takes wind_scale_host as femfct_schnak_forward_tw (NULL: stationary wind). */
int femfct_nonlinear_forward_ct(femfct_ctx* ctx, const double* Aw_ell, const double* c_traj, int32_t c_shared,
                                double* u_traj, int32_t num_steps, double dt, double eps, int32_t batch);
int femfct_schnak_forward_ct(femfct_ctx* ctx, const double* Aw_ell, const double* wind_scale_host, const double* c_traj,
                             int32_t c_shared, double* u_traj, double* v_traj, int32_t num_steps, double dt,
                             const double* par, double rescaling, int32_t batch);
int femfct_chtxs_forward_ct(femfct_ctx* ctx, const double* c_traj, int32_t c_shared, double* u_traj, double* v_traj,
                            int32_t num_steps, double dt, const double* par, double rescaling, int32_t batch);
/* Chemotaxis with cell growth (Mimura-Tsujikawa): du/dt + div(-Dm grad u + chi u exp(-eta u) grad v) = r(u),
 * r(u) = u (r0 + r1 u + r2 u^2), growth = {r0, r1, r2}: {4, -1, 0} is m (4 - m) (chemotaxis_mimura_FCT_PGD_alltime.py, header),
 * {0, 1, -1} is m^2 (1 - m) (mimura_data_helpers.py:70).  IMEX as the reference runs it: the FCT step from level n to n+1
 * gets rhs = assemble(r(u_n)*v*dx), and the adjoint p step to level n gains assemble(r'(u_n)*p_{n+1}*w*dx) on its
 * right-hand side (explicit, like the c_n q_{n+1} term); the v / q equations, the terminal conditions and the misfits are
 * unchanged.  growth = NULL (or all three zero): exactly the sweeps above; a coefficient that is not finite is
 * FEMFCT_ERR_INVALID.  femfct_chtxs_forward_g: c_per_step = 0: c is the frozen control level (femfct_chtxs_forward,
 * c_shared ignored), != 0: a control trajectory (femfct_chtxs_forward_ct). */
int femfct_chtxs_forward_g(femfct_ctx* ctx, const double* c, int32_t c_per_step, int32_t c_shared, double* u_traj,
                           double* v_traj, int32_t num_steps, double dt, const double* par, double rescaling,
                           const double* growth, int32_t batch);
int femfct_chtxs_adjoint_g(femfct_ctx* ctx, const double* u_traj, const double* v_traj, const double* uhat,
                           const double* vhat, double* p_traj, double* q_traj, const double* c_traj, int32_t num_steps,
                           double dt, const double* par, double rescaling, int32_t alltime, const double* growth,
                           int32_t batch);
/* Snapshot observations for the three PDE systems (added after ABI version 5, backward compatible): the adjoint sweeps of
 *   J = 1/2 sum_n w^u_n ||u_n - uhat_n||^2_Mw + 1/2 sum_n w^v_n ||v_n - vhat_n||^2_Mw + beta/2 ||c||^2_Q,
 * Mw = assemble(omega_h*u*v*dx) (M without a window).  uhat/vhat_traj: (num_steps + 1)*n doubles per member, read at observed
 * levels only.  theta_*_dev: num_steps + 1 doubles on the device, read per level inside the captured step (the values may
 * change between sweeps); NULL: the variable is not observed and its target may be NULL.  Terminal conditions
 * p_Nt = tau_u omega .* (uhat_Nt - u_Nt), q_Nt = tau_v omega .* (vhat_Nt - v_Nt), always written (zeros for tau = 0, the
 * target's last level unread); the step to level n gains (theta_n/dt) Mw (hat_n - state_n) in the launches that carry the
 * all-time misfits.  (tau, theta) = (1, 0) and (0, dt) without a window give the bits of the final-time and all-time sweeps;
 * for chemotaxis with misfit = FEMFCT_MISFIT_NODAL, which loads (theta_n/dt) omega .* (hat_n - state_n) as helpers.py:1506-1507,
 * 1533-1534 do; FEMFCT_MISFIT_MASS is the discrete adjoint load of J.  window_dev: n doubles or NULL.  A tau that is not
 * finite or an unknown misfit: FEMFCT_ERR_INVALID.  Sweep kinds and budgets are those of the systems' adjoint sweeps (the
 * nonlinear equation: its all-time kind). */
#define FEMFCT_MISFIT_NODAL 0
#define FEMFCT_MISFIT_MASS 1
int femfct_nonlinear_adjoint_obs(femfct_ctx* ctx, const double* Aw_ell, const double* u_traj, const double* uhat_traj,
                                 const double* theta_u_dev, double tau_u, const double* window_dev, double* p_traj,
                                 int32_t num_steps, double dt, double eps, int32_t batch);
/* wind_scale_host: as in femfct_schnak_adjoint_tw, NULL: stationary wind */
int femfct_schnak_adjoint_obs(femfct_ctx* ctx, const double* AwT_ell, const double* wind_scale_host, const double* u_traj,
                              const double* v_traj, const double* uhat_traj, const double* vhat_traj,
                              const double* theta_u_dev, double tau_u, const double* theta_v_dev, double tau_v,
                              const double* window_dev, double* p_traj, double* q_traj, int32_t num_steps, double dt,
                              const double* par, int32_t batch);
/* growth: as in femfct_chtxs_adjoint_g, NULL: none */
int femfct_chtxs_adjoint_obs(femfct_ctx* ctx, const double* u_traj, const double* v_traj, const double* uhat_traj,
                             const double* vhat_traj, const double* theta_u_dev, double tau_u, const double* theta_v_dev,
                             double tau_v, const double* window_dev, double* p_traj, double* q_traj, const double* c_traj,
                             int32_t num_steps, double dt, const double* par, double rescaling, const double* growth,
                             int32_t misfit, int32_t batch);
/* all-time misfit of the nonlinear equation (nonlinear_FCT_PDECO_alltime.py:198-216 with the HEAD operators of
 * helpers.py:1017-1037): p(T) = 0; for n = Nt-1..0:
 *   p_n = FCT_alg_ref(-Mat_p, M (uhat_n - u_n), p_{n+1}, non_flux_mat = M_u2(u_n) - M)
 * uhat_traj: (num_steps+1)*n doubles per member (batch stride (num_steps+1)*n), uhat_shared != 0: one trajectory for
 * the whole batch. */
int femfct_nonlinear_adjoint_alltime(femfct_ctx* ctx, const double* Aw_ell, const double* u_traj,
                                     const double* uhat_traj, int32_t uhat_shared, double* p_traj,
                                     int32_t num_steps, double dt, double eps, int32_t batch);
/* BiCGStab diagnostics of the most recent sweep that used it: info_host[step*batch + b] */
int femfct_traj_krylov_info(femfct_ctx* ctx, femfct_step_info* info_host, int32_t num_steps, int32_t batch);

#ifdef __cplusplus
}
#endif
#endif /* FEMFCT_H */
