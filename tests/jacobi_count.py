"""How many plain Jacobi sweeps the low-order system of an oracle step needs (pure NumPy / SciPy on the oracle).

The device solves L x = b, L = M_L + dt (A - D) [+ dt N], b = M_L u_n + dt rhs, by Jacobi sweeps from x0 = b / diag(L)
(k_build_low) until ||b - L x||_inf <= rel_tol ||b||_inf (femfct_set_solver; rel_tol = 1e-13).  ``sweeps`` runs exactly that
on the oracle's own operator (``oracle.fct.fct_step(..., info=)["l_vals"]`` on ``Pattern.csr``), so the tests of the sweep
controller (tests/test_gpu_sweep_controller.py) can choose inputs whose solve lies above the controller's starting
budgets, and tests/test_jacobi_count.py can hold every such input to the window its case needs.

The counts pick inputs; they are no tolerances.  Fused launches report whole launches and the one-workgroup step sweeps
Gauss-Seidel inside a thread's block (fewer sweeps than plain Jacobi), so a device log is compared with these counts
only through the budgets the inputs were chosen against.

The second half holds the solid-body inputs of those tests, shared by both files so that the CPU test pins what the GPU
test runs."""
import numpy as np

from oracle import traj as otraj
from oracle.assembly import P1Assembler
from oracle.mesh import SquareMesh

REL_TOL = 1e-13
START_BUDGET, START_BUDGET_MESH, START_KBUDGET, MAX_ITERS = 48, 96, 40, 400   # femfct_run_sweep / femfct_set_solver


def low_order_system(cm, A, rhs, u_n, dt, non_flux_mat=None):
    """(L, b, info) of the oracle step ``cm.fct(A, rhs, u_n, dt, non_flux_mat)``; info is fct_step's (u_low, l_rowsum, ..)."""
    info = {}
    cm.fct(A, rhs, u_n, dt, non_flux_mat=non_flux_mat, info=info)
    L = cm.pat.csr(info["l_vals"])
    b = cm.ml * np.asarray(u_n, dtype=np.float64) + dt * np.asarray(rhs, dtype=np.float64)
    return L, b, info


def sweeps(L, b, rel_tol=REL_TOL, max_sweeps=4000):
    """(count, x): plain Jacobi sweeps from x0 = b / diag(L) until ||b - L x||_inf <= rel_tol ||b||_inf, and the iterate
    that met it.  count = max_sweeps + 1 when none did (x is then the last iterate)."""
    d = L.diagonal()
    x = b / d
    bound = rel_tol * np.abs(b).max()
    for k in range(max_sweeps + 1):
        r = b - L @ x
        if np.abs(r).max() <= bound:
            return k, x
        if k < max_sweeps:
            x = x + r / d
    return max_sweeps + 1, x


def count_step(cm, A, rhs, u_n, dt, non_flux_mat=None, **kw):
    """(count, rowsum_ok, x, info) of one oracle step: the Jacobi sweep count of its low-order solve, the reference's
    M-matrix diagnostic min_i sum_j L_ij > 0 (helpers.py:1796), the converged iterate and fct_step's info."""
    L, b, info = low_order_system(cm, A, rhs, u_n, dt, non_flux_mat)
    k, x = sweeps(L, b, **kw)
    return k, bool(np.asarray(L.sum(axis=1)).min() > 0), x, info


# ----------------------------------------------------------------------------- the solid-body inputs of the controller tests
_SB = {}


def solid_body(N):
    """(mesh, asm, SolidBody) of the oracle on [-1, 1]^2 with N nodes per side (om = pi / 40, eps = 0), one mesh kept"""
    if N not in _SB:
        mesh = SquareMesh(-1.0, 1.0, N - 1)
        asm = P1Assembler(mesh)
        _SB.clear()
        _SB[N] = (mesh, asm, otraj.SolidBody(asm))
    return _SB[N]


def control_shape(mesh):
    """1 + 0.5 sin 3x cos 2y in FEniCS DoF order: smooth, so that L stays column-dominant and plain Jacobi contracts"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    return 1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)


def state(mesh, seed):
    """exp(-20 ((x + 0.3)^2 + (y - 0.2)^2)) + 0.01 rand in FEniCS DoF order"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    return np.exp(-20 * ((x + 0.3) ** 2 + (y - 0.2) ** 2)) + 0.01 * np.random.default_rng(seed).random(mesh.nodes)


def control_traj(mesh, amps):
    """level k of the control = amps[k] * control_shape (len(amps) = Nt + 1), level-major"""
    return (np.asarray(amps, dtype=np.float64)[:, None] * control_shape(mesh)[None, :]).ravel()


def solid_body_counts(N, dt, amp, seed=0):
    """{"forward": (count, rowsum_ok), "adjoint": (count, rowsum_ok)} of one solid-body step with the control
    amp * control_shape: the forward operator -A_u and the adjoint operator -A_p (oracle.traj.solidbody_*)."""
    mesh, asm, sb = solid_body(N)
    c = amp * control_shape(mesh)
    u = state(mesh, seed)
    A_u = sb.A_u(c)
    A_p = -sb.eps * sb.cm.Ad - sb.Arot - asm.drift1(c, sb.drift) - asm.drift2(c, sb.drift)
    zero = np.zeros(mesh.nodes)
    return {"forward": count_step(sb.cm, -A_u, zero, u, dt)[:2], "adjoint": count_step(sb.cm, -A_p, zero, u, dt)[:2]}


# (N, dt, amp) of every input set of tests/test_gpu_sweep_controller.py and the window (lo, hi) its case needs:
# lo < forward count < hi and lo < adjoint count < hi.  "hard" lies above the starting budget of its regime and below
# the sweep cap; "easy" below the starting budget; the one-workgroup step needs about 0.7 x the plain-Jacobi count
# (DESIGN 4 (iii)), so its hard inputs lie above 96 / 0.7 = 138; its easy ones lie under 96 plain sweeps (the GPU test
# asserts on the device log which side of the cap each landed on).
WINDOWS = {
    # 81 x 81 (tile32, patch64), dt = 2.5e-3
    ("N81", 0.0): (81, 2.5e-3, 0.0, (START_BUDGET, MAX_ITERS)),
    ("N81", 3.0): (81, 2.5e-3, 3.0, (START_BUDGET, MAX_ITERS)),
    ("N81", 10.0): (81, 2.5e-3, 10.0, (START_BUDGET, MAX_ITERS)),
    ("N81", 30.0): (81, 2.5e-3, 30.0, (100, MAX_ITERS)),
    # 81 x 81, dt = 1e-3: under the starting budget; amp 0 passes the row-sum diagnostic, amp >= 1 fails it
    ("N81-easy", 0.0): (81, 1e-3, 0.0, (0, START_BUDGET)),
    ("N81-easy", 3.0): (81, 1e-3, 3.0, (0, START_BUDGET)),
    ("N81-easy", 10.0): (81, 1e-3, 10.0, (0, START_BUDGET)),
    # 41 x 41 in FEniCS order (rows, strips), dt = 5e-3
    ("N41", 0.0): (41, 5e-3, 0.0, (START_BUDGET, MAX_ITERS)),
    ("N41", 3.0): (41, 5e-3, 3.0, (START_BUDGET, MAX_ITERS)),
    ("N41", 10.0): (41, 5e-3, 10.0, (START_BUDGET, MAX_ITERS)),
    ("N41", 30.0): (41, 5e-3, 30.0, (START_BUDGET, MAX_ITERS)),
    # 41 x 41 in vertex order (2 x 2 one-workgroup step), dt = 1e-2
    ("N41-mesh", 0.0): (41, 1e-2, 0.0, (START_BUDGET, START_BUDGET_MESH)),
    ("N41-mesh", 50.0): (41, 1e-2, 50.0, (138, MAX_ITERS)),
    # 41 x 41, dt = 2e-3: under the starting budget; amp 0 alone passes the row-sum diagnostic
    ("N41-easy", 0.0): (41, 2e-3, 0.0, (0, START_BUDGET)),
    ("N41-easy", 3.0): (41, 2e-3, 3.0, (0, START_BUDGET)),
    ("N41-easy", 10.0): (41, 2e-3, 10.0, (0, START_BUDGET)),
    # 81 x 81, 64 members (3 x 3 one-workgroup step), dt = 4e-3
    ("N81-mesh", 0.0): (81, 4e-3, 0.0, (START_BUDGET, START_BUDGET_MESH)),
    ("N81-mesh", 40.0): (81, 4e-3, 40.0, (138, MAX_ITERS)),
}
