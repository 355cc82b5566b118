"""CPU reference of the all-time adjoint of the nonlinear equation (femfct_nonlinear_adjoint_alltime,
``solve_adjoint_nonlinear_equation(optim="alltime")``), built from the unchanged oracle.

nonlinear_FCT_PDECO_alltime.py:198-216 with the HEAD operators of helpers.py:1017-1037: p(T) = 0, and for
n = Nt-1..0

    p_n = FCT(-Mat_p, M (uhat_n - u_n), p_{n+1}, non_flux_mat = M_u2(u_n) - M),    Mat_p = -A - eps Ad.

The misfit load is ``cm.M @ (uhat_n - u_n)``, as the oracle's Schnakenberg all-time branch writes it (oracle/traj.py:212).
The script assembles M_u2 from the level it has just zeroed (:187-191) and reuses that stale matrix in its adjoint (:216);
this reference takes HEAD's M_u2(u_n), as the device does.

``solve_adjoint_nonlinear_equation`` keeps the signature of ``oracle.traj.solve_adjoint_nonlinear_equation`` (``uhat_T``
is the target trajectory here), so that it can stand in for it inside ``oracle.pdeco.projected_gradient_descent``
(with ``per_step_oracle.solve_nonlinear_equation`` for the state: the script's per-step control)."""
import numpy as np

from oracle.traj import _common, nonlinear_params, nonlinear_wind


def solve_adjoint_nonlinear_equation(uk, uhat_T, pk, T, asm, nodes, num_steps, dt, dof_neighbors=None):
    cm = _common(asm)
    P = nonlinear_params()
    A = asm.convection(nonlinear_wind)
    Mat_p = -A - P["eps"] * cm.Ad
    pk[num_steps * nodes:] = 0.0                   # pk = np.zeros(vec_length) (:200)
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        pk_np1 = pk[end:end + nodes]
        uk_n = uk[start:end]
        M_u2 = asm.weighted_mass(lambda at: at(uk_n) ** 2)
        Mat_rhs = M_u2 - cm.M
        rhs = cm.M @ (uhat_T[start:end] - uk_n)
        pk[start:end] = cm.fct(-Mat_p, rhs, pk_np1, dt, non_flux_mat=Mat_rhs)
    return pk


def sinsin_control(mesh, num_steps):
    """c = sin(2 pi x) sin(2 pi y) on every level, FEniCS DoF order: the control of the target generator
    nonlinear_generate_pattern_FCT.py:48-50, 83-85, 92-93"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    return np.tile(np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y), num_steps + 1)
