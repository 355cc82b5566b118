"""CPU reference of the chemotaxis sweeps with a cell-growth term, restated from the oracle's pieces.

    du/dt + div(-Dm grad u + chi u exp(-eta u) grad v) = r(u),   r(u) = u (r0 + r1 u + r2 u^2),   growth = (r0, r1, r2)

The two loops are those of ``oracle.traj.solve_chtxs_system`` / ``solve_adjoint_chtxs_system`` (oracle/traj.py:221-278) with
two more load vectors, both explicit in time (IMEX, as mimura_data_helpers.py:65-70 runs the reaction term):

    forward   the FCT step from level n to n+1 gets  rhs_i = int r(u_n,h) phi_i         in place of zeros,
    adjoint   the p step to level n gains            int r'(u_n,h) p_{n+1,h} phi_i,     r'(u) = r0 + 2 r1 u + 3 r2 u^2.

Both integrands have degree 4 and ``asm.load`` integrates them with the 7-point degree-5 rule: exactly.  ``growth=None``
adds nothing, and the zero growth adds vectors of zeros: either way the bits of the oracle's own loops.  ``per_step``:
the step to level n+1 reads control level n+1 (tests/per_step_oracle.py) instead of the frozen level 1.  The signatures
are the oracle's, so that :func:`patched` can put these functions in their place inside
``oracle.pdeco.projected_gradient_descent``, which calls them through ``traj.``."""
import contextlib
import functools

import numpy as np
from scipy.sparse.linalg import spsolve

from oracle import traj as otraj
from oracle.traj import _common, chtxs_params


def r(u, growth):
    r0, r1, r2 = growth
    return u * (r0 + r1 * u + r2 * u * u)


def dr(u, growth):
    r0, r1, r2 = growth
    return r0 + 2 * r1 * u + 3 * r2 * u * u


def solve_chtxs_system(control, var1, var2, asm, nodes, num_steps, dt, dof_neighbors=None, control_const=None,
                       rescaling=1 / 10, growth=None, per_step=False):
    cm = _common(asm)
    P = chtxs_params()
    delta, Dm, Df, chi, eta = P["delta"], P["Dm"], P["Df"], P["chi"], P["eta"]
    Mat_var2 = (cm.M + dt * (Df * cm.Ad + delta * cm.M)).tocsc()
    var1[nodes:] = np.zeros(num_steps * nodes)
    var2[nodes:] = np.zeros(num_steps * nodes)
    frozen = None
    for i in range(1, num_steps + 1):
        start, end = i * nodes, (i + 1) * nodes
        u_n = var1[start - nodes:start]
        v_n = var2[start - nodes:start]
        if frozen is None or (per_step and control_const is None):
            frozen = (np.full(nodes, float(control_const)) if control_const is not None
                      else control[start:end].copy())
        rhs2 = asm.load(lambda at: at(v_n) + dt * at(frozen) * at(u_n) / rescaling)
        v_np1 = spsolve(Mat_var2, rhs2)
        var2[start:end] = v_np1
        Aa = asm.chtxs_forward_Aa(u_n, v_np1, eta)
        A_var1 = Dm * cm.Ad - chi * Aa
        rhs1 = np.zeros(nodes)
        if growth is not None:
            rhs1 = rhs1 + asm.load(lambda at: r(at(u_n), growth))
        var1[start:end] = cm.fct(A_var1, rhs1, u_n, dt)
    return var1, var2


def solve_adjoint_chtxs_system(uk, vk, uhat, vhat, pk, qk, control, T, asm, nodes, num_steps, dt, dof_neighbors=None,
                               optim="alltime", rescaling=1 / 10, growth=None, drop_adjoint_load=False):
    """``drop_adjoint_load``: leave the r'(u) p load out (what a wrong adjoint would do; the gradient test uses it to
    show that its bound notices)."""
    if optim not in ("alltime", "finaltime"):
        raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of ['alltime', 'finaltime'].")
    cm = _common(asm)
    P = chtxs_params()
    delta, Dm, Df, chi, eta = P["delta"], P["Dm"], P["Df"], P["chi"], P["eta"]
    if optim == "finaltime":
        pk[num_steps * nodes:] = uhat - uk[num_steps * nodes:]
        qk[num_steps * nodes:] = vhat - vk[num_steps * nodes:]
    Mat_q = (cm.M + dt * (Df * cm.Ad + delta * cm.M)).tocsc()
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        q_np1 = qk[end:end + nodes]
        p_np1 = pk[end:end + nodes]
        u_n = uk[start:end]
        v_n = vk[start:end]
        c_n = control[start:end]
        Aa = asm.chtxs_adjoint_Aa(u_n, v_n, eta)
        Mat_p = Dm * cm.Ad - chi * Aa
        rhs_p = asm.load(lambda at: at(c_n) * at(q_np1) / rescaling)
        if optim == "alltime":
            rhs_p = rhs_p + (uhat[start:end] - uk[start:end])
        if growth is not None and not drop_adjoint_load:
            rhs_p = rhs_p + asm.load(lambda at: dr(at(u_n), growth) * at(p_np1))
        pk[start:end] = cm.fct(Mat_p, rhs_p, p_np1, dt)
        p_n = pk[start:end]
        rhs_q = asm.chtxs_adjoint_rhs_q(u_n, p_n, chi, eta)
        if optim == "alltime":
            rhs_q = rhs_q + (vhat[start:end] - vk[start:end])
        qk[start:end] = spsolve(Mat_q, cm.M @ q_np1 + dt * rhs_q)
    return pk, qk


@contextlib.contextmanager
def patched(growth, per_step):
    """``oracle.traj``'s chemotaxis sweeps replaced by the ones above for the duration of the block"""
    saved = otraj.solve_chtxs_system, otraj.solve_adjoint_chtxs_system
    otraj.solve_chtxs_system = functools.partial(solve_chtxs_system, growth=growth, per_step=per_step)
    otraj.solve_adjoint_chtxs_system = functools.partial(solve_adjoint_chtxs_system, growth=growth)
    try:
        yield
    finally:
        otraj.solve_chtxs_system, otraj.solve_adjoint_chtxs_system = saved
