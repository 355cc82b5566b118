"""CPU reference of snapshot tracking (``solvers.Observations``) for the solid-body / linear family, a loop built from
the unchanged oracle's pieces: ``oracle.traj.solidbody_forward``, the oracle's FCT step, its mass matrix and its P1 load.

    J = 1/2 sum_n w_n (u_n - uhat_n)^T Mw (u_n - uhat_n) + beta/2 ||c||^2_Q,      Mw = assemble(omega_h u v dx)

    adjoint   p_Nt = tau * omega .* (uhat_Nt - u_Nt),    rhs_n = (theta_n / dt) assemble(omega_h (uhat_n - u_n) v dx)
              [- Mg(g_n) p_{n+1}],    p_n = FCT_alg_ref(-A_p(c_n), rhs_n, p_{n+1})

With (tau, theta) = (1, 0) and (0, dt) these are the statements of ``oracle.traj.solidbody_adjoint`` for "finaltime" and
"alltime", operation for operation (theta_n/dt = 1 and a factor omega = 1 are exact), so the results have its bits.  The
load is the oracle's quadrature load (exact: a cubic integrand under the degree-5 rule); ``weighted_mass`` assembles Mw
from the exact P1 triple products int_K phi_a phi_b phi_c = |K|/60 {6, 2, 1}, the product the device kernels apply --
the two agree to rounding (test_snapshots_oracle.py).  A level of zero weight is not read: ``uhat`` may hold NaN there.
``step="low"`` runs the low-order (linear, unlimited) solve of the FCT step in place of the limited one."""
import numpy as np

from oracle import traj as otraj
from oracle.fct import l2_norm_sq_Q

_TRIPLE = np.ones((3, 3, 3))
for _a in range(3):
    for _b in range(3):
        _TRIPLE[_a, _a, _b] = _TRIPLE[_a, _b, _a] = _TRIPLE[_b, _a, _a] = 2.0
    _TRIPLE[_a, _a, _a] = 6.0


def weighted_mass(asm, omega):
    """assemble(omega_h u v dx) for nodal values ``omega`` (DoF order) from the exact triple products"""
    loc = np.asarray(omega, dtype=np.float64)[asm.dof]                      # (nt, 3)
    Ke = (asm.area / 60.0)[:, None, None] * np.einsum("ijk,tk->tij", _TRIPLE, loc)
    return asm._mat(Ke)


def misfit_load(asm, d, omega=None):
    """assemble(omega_h d_h v dx) the way the oracle's all-time sweep assembles its load (alltime.py:257)"""
    if omega is None:
        return asm.load(lambda at: at(d))
    return asm.load(lambda at: at(omega) * at(d))


def _step(sb, A, rhs, p_np1, dt, step):
    if step == "fct":
        return sb.cm.fct(A, rhs, p_np1, dt)
    info = {}
    sb.cm.fct(A, rhs, p_np1, dt, info=info)
    return info["u_low"]


def adjoint(sb, ck, uk, uhat, obs, nodes, num_steps, dt, step="fct", Mg=None, A_p=None):
    """The adjoint sweep for the observations ``obs`` (anything with theta, tau, window).  ``A_p``: a fixed adjoint
    operator (the linear problems) instead of the drift-control one; ``Mg(level)``: the reaction matrices."""
    n, Nt = nodes, num_steps
    pk = np.zeros((Nt + 1) * n)
    w = obs.window
    if obs.tau != 0.0:
        d = uhat[Nt * n:] - uk[Nt * n:]
        pk[Nt * n:] = obs.tau * (d if w is None else w * d)
    for i in reversed(range(0, Nt)):
        start, end = i * n, (i + 1) * n
        p_np1 = pk[end:end + n]
        if A_p is None:
            c_n = ck[start:end]
            A = -sb.eps * sb.cm.Ad - sb.Arot - sb.asm.drift1(c_n, sb.drift) - sb.asm.drift2(c_n, sb.drift)
        else:
            A = A_p
        if obs.theta[i] != 0.0:
            u_n, uh_n = uk[start:end], uhat[start:end]
            if w is None:
                load = sb.asm.load(lambda at: at(uh_n) - at(u_n))              # alltime.py:257
            else:
                load = sb.asm.load(lambda at: at(w) * (at(uh_n) - at(u_n)))
            rhs = (obs.theta[i] / dt) * load
        else:
            rhs = np.zeros(n)
        if Mg is not None:
            rhs = rhs - Mg(i) @ p_np1
        pk[start:end] = _step(sb, -A, rhs, p_np1, dt, step)
    return pk


def misfit(asm, M, uk, uhat, obs, nodes):
    """1/2 sum_n cost_w[n] (u_n - uhat_n)^T Mw (u_n - uhat_n), levels of zero weight unread"""
    Mw = M if obs.window is None else weighted_mass(asm, obs.window)
    J = 0.0
    for lv in np.flatnonzero(obs.cost_w):
        d = uk[lv * nodes:(lv + 1) * nodes] - uhat[lv * nodes:(lv + 1) * nodes]
        J = J + obs.cost_w[lv] * (d @ (Mw @ d))
    return 0.5 * J


def cost(sb, uk, uhat, ck, obs, nodes, num_steps, dt, beta):
    return misfit(sb.asm, sb.cm.M, uk, uhat, obs, nodes) + beta / 2 * l2_norm_sq_Q(ck, num_steps, dt, sb.cm.M)


def pgd_loop(sb, u0, uhat, obs, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, gam=1e-4, s0=1.0, max_armijo=10):
    """``oracle.traj.solidbody_pgd_loop`` with the adjoint and the cost above; u is seeded with the target at the
    observed levels past level 0, as that loop seeds it in its two modes.  Same history."""
    n, Nt = nodes, num_steps
    tl = (Nt + 1) * n
    uhat = np.asarray(uhat, dtype=np.float64)
    uk = np.zeros(tl)
    uk[:n] = u0
    for lv in obs.levels:
        if lv > 0:
            uk[lv * n:(lv + 1) * n] = uhat[lv * n:(lv + 1) * n]
    c_prev = np.array(c0, dtype=np.float64)
    pk = np.zeros(tl)
    hist = dict(cost=[], armijo_k=[], armijo_margin=[])
    for _ in range(iters):
        pk = adjoint(sb, c_prev, uk, uhat, obs, n, Nt, dt)
        dk = otraj.solidbody_descent_direction(sb, c_prev, uk, pk, beta, n, Nt)
        ck = np.clip(c_prev + s0 * dk, c_lower, c_upper)
        otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
        J_k = cost(sb, uk, uhat, ck, obs, n, Nt, dt, beta)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            c_inc = np.clip(ck + s * dk, c_lower, c_upper)
            otraj.solidbody_forward(sb, c_inc, uk, n, Nt, dt)
            J = cost(sb, uk, uhat, c_inc, obs, n, Nt, dt, beta)
            stat = l2_norm_sq_Q(c_inc - ck, Nt, dt, sb.cm.M)
            margins.append((J - J_k + gam / s * stat) / abs(J_k))
            if not (J - J_k > -gam / s * stat):
                break
        hist["cost"].append(J)
        hist["armijo_k"].append(k + 1)
        hist["armijo_margin"].append(margins)
        c_prev = c_inc
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return uk, pk, c_prev, hist
