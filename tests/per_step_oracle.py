"""CPU reference of the per-step control mode (``control_per_step=True``), built from the unchanged oracle.

One oracle step from u_k with ``control = [., c_{k+1}]`` and ``num_steps = 1`` is one per-step step: the oracle freezes
``control[nodes:2 * nodes]``, which is then exactly c_{k+1}.  Chaining Nt such calls gives the per-step trajectory.  A
time-dependent Schnakenberg wind is shifted, ``lambda t: s(t_k + t)``, with t_k accumulated as the oracle accumulates
its own time (``t += dt``), so that ``t_k + dt`` has the bits of the single call's ``t``.

The chained functions keep the oracle's signatures (``oracle.traj.solve_*``), so that they can stand in for them inside
``oracle.pdeco.projected_gradient_descent``; the oracle's own functions are bound here at import time."""
import numpy as np

from oracle.traj import solve_chtxs_system as _chtxs
from oracle.traj import solve_nonlinear_equation as _nonlinear
from oracle.traj import solve_schnak_system as _schnak


def _two_levels(x, k, nodes):
    """[x_k, 0] (state) -- or, for the control, [., x_{k+1}]: level k+1 in the slot the oracle reads"""
    return np.concatenate([x[k * nodes:(k + 1) * nodes], np.zeros(nodes)])


def _control(control, k, nodes):
    out = np.zeros(2 * nodes)
    out[nodes:] = control[(k + 1) * nodes:(k + 2) * nodes]
    return out


def solve_nonlinear_equation(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors=None, control_const=None):
    if control_const is not None:
        return _nonlinear(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors, control_const)
    var1[nodes:] = 0.0
    for k in range(num_steps):
        u = _two_levels(var1, k, nodes)
        _nonlinear(_control(control, k, nodes), u, None, asm, nodes, 1, dt, dof_neighbors)
        var1[(k + 1) * nodes:(k + 2) * nodes] = u[nodes:]
    return var1, None


def solve_schnak_system(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors=None, control_const=None,
                        rescaling=1, wind=None, wind_scale=None):
    if control_const is not None:
        return _schnak(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors, control_const, rescaling, wind,
                       wind_scale)
    var1[nodes:] = 0.0
    var2[nodes:] = 0.0
    t_k = 0.0
    for k in range(num_steps):
        u, v = _two_levels(var1, k, nodes), _two_levels(var2, k, nodes)
        ws = None if wind_scale is None else (lambda t, t0=t_k: wind_scale(t0 + t))
        _schnak(_control(control, k, nodes), u, v, asm, nodes, 1, dt, dof_neighbors, None, rescaling, wind, ws)
        var1[(k + 1) * nodes:(k + 2) * nodes] = u[nodes:]
        var2[(k + 1) * nodes:(k + 2) * nodes] = v[nodes:]
        t_k += dt
    return var1, var2


def solve_chtxs_system(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors=None, control_const=None,
                       rescaling=1 / 10):
    if control_const is not None:
        return _chtxs(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors, control_const, rescaling)
    var1[nodes:] = 0.0
    var2[nodes:] = 0.0
    for k in range(num_steps):
        u, v = _two_levels(var1, k, nodes), _two_levels(var2, k, nodes)
        _chtxs(_control(control, k, nodes), u, v, asm, nodes, 1, dt, dof_neighbors, None, rescaling)
        var1[(k + 1) * nodes:(k + 2) * nodes] = u[nodes:]
        var2[(k + 1) * nodes:(k + 2) * nodes] = v[nodes:]
    return var1, var2


# ----------------------------------------------------------------------------- the test problems
def bump(mesh):
    """a smooth bump inside the unit square, in FEniCS DoF order"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    return np.exp(-((x - 0.45) ** 2 + (y - 0.55) ** 2) / 0.04)


def varying_control(cbar, num_steps, amp=0.5, phase=0.0):
    """c_k(x) = cbar(x) * (1 + amp*sin(2 pi k / Nt + phase)), k = 0..Nt, level-major"""
    k = np.arange(num_steps + 1)[:, None]
    return (cbar[None, :] * (1.0 + amp * np.sin(2 * np.pi * k / num_steps + phase))).ravel()


def constant_control(cbar, num_steps):
    return np.tile(cbar, num_steps + 1)


# control amplitude of each system (of the order the drivers use: DEFAULTS' box constraints)
SCALE = {"nonlinear": 1.0, "schnak": 0.1, "chtxs": 10.0}


def sin_wind(t):
    """s(t) of the wind of Schnak_FCT_PDECO_alltime.py:55 (sin(2 pi t))"""
    return np.sin(2 * np.pi * t)


def initial_conditions(problem, mesh):
    """(u0,) / (u0, v0) in FEniCS DoF order: the shapes of helpers.py's ICs (nonlinear_equation_IC, schnak_sys_IC), and
    for chemotaxis a smooth perturbation of its constant state"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    if problem == "nonlinear":
        return (5 * y * (y - 1) * x * (x - 1) * np.sin(4 * np.pi * x),)
    if problem == "schnak":
        pert = 0.01 * sum(np.cos(2 * np.pi * x * i) for i in range(1, 9))
        return 1.0 + 0.1 * np.cos(2 * np.pi * (x + y)) + pert, 0.9 + 0.1 * np.cos(2 * np.pi * (x + y)) + pert
    u0 = 1.5 + 0.05 * np.cos(3 * np.pi * x) * np.cos(2 * np.pi * y)
    return u0, u0.copy()
