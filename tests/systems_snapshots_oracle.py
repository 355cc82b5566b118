"""CPU reference of snapshot tracking (``solvers.Observations``) for the nonlinear, Schnakenberg and chemotaxis systems,
restated from the oracle's pieces as tests/snapshots_oracle.py and tests/chtxs_growth_oracle.py are.

    J = 1/2 sum_n w^u_n ||u_n - uhat_n||^2_Mw + 1/2 sum_n w^v_n ||v_n - vhat_n||^2_Mw + beta/2 ||c||^2_Q

The loops are those of ``oracle.traj.solve_adjoint_{nonlinear_equation,schnak_system,chtxs_system}`` (the chemotaxis one
with the growth load of chtxs_growth_oracle.py) with the terminal conditions and misfit loads of the observations:

    p_Nt = tau^u omega .* (uhat_Nt - u_Nt),  q_Nt = tau^v omega .* (vhat_Nt - v_Nt)     (zeros for tau = 0 / not observed)
    nonlinear     rhs_n  = (theta_n/dt) Mw (uhat_n - u_n)
    Schnakenberg  rhs_q += (theta^v_n/dt) Mw (vhat_n - v_n),   rhs_p += (theta^u_n/dt) Mw (uhat_n - u_n)
    chemotaxis    misfit="mass":  the same two terms;   misfit="nodal":  omega .* ( ) in the place of Mw ( )

Mw = M without a window, else the exact P1 triple-product matrix of snapshots_oracle.weighted_mass.  A level of zero
weight is not read: the targets may hold NaN there, and an unobserved variable's target may be None.  With
``Observations.finaltime`` / ``.alltime`` (theta_n/dt = 1 exactly) and no window the statements are the oracle's, operation
for operation (chemotaxis: ``misfit="nodal"``), so the results have its bits.  ``drop_loads``: leave the interior misfit
loads out (what a wrong adjoint would do).  ``step="low"`` runs the low-order (linear, unlimited) solve of the FCT step in
place of the limited one, as snapshots_oracle.adjoint does."""
import numpy as np
from scipy.sparse.linalg import spsolve

import chtxs_growth_oracle as go
import snapshots_oracle as so
from oracle.fct import l2_norm_sq_Q
from oracle.traj import _common, chtxs_params, nonlinear_params, nonlinear_wind, schnak_params, schnak_wind


def pair(obs):
    """(obs_u, obs_v) of one Observations for both variables or a pair with at most one None"""
    return tuple(obs) if isinstance(obs, (tuple, list)) else (obs, obs)


def _window(ou, ov):
    o = ou if ou is not None else ov
    return o.window


def _terminal(o, hat, state, nodes, Nt):
    if o is None or o.tau == 0.0:
        return np.zeros(nodes)
    d = hat[Nt * nodes:] - state[Nt * nodes:]
    return o.tau * (d if o.window is None else o.window * d)


class _Misfit:
    """the load (theta_n/dt) [Mw | omega .*] (hat_n - state_n) of one variable, zeros (nothing read) at theta_n = 0"""

    def __init__(self, asm, M, o, dt, mass=True, drop=False):
        self.o, self.dt, self.mass, self.drop = o, dt, mass, drop
        w = None if o is None else o.window
        self.w = w
        self.Mw = M if w is None else so.weighted_mass(asm, w)

    def __call__(self, i, hat, state, nodes):
        o = self.o
        if o is None or o.theta[i] == 0.0 or self.drop:
            return None
        d = hat[i * nodes:(i + 1) * nodes] - state[i * nodes:(i + 1) * nodes]
        if self.mass:
            return (o.theta[i] / self.dt) * (self.Mw @ d)
        return (o.theta[i] / self.dt) * (d if self.w is None else self.w * d)


def _fct(cm, A, rhs, x, dt, step, **kw):
    if step == "fct":
        return cm.fct(A, rhs, x, dt, **kw)
    info = {}
    cm.fct(A, rhs, x, dt, info=info, **kw)
    return info["u_low"]


def _add(rhs, load):
    return rhs if load is None else rhs + load


def solve_adjoint_nonlinear_equation(uk, uhat, pk, T, asm, nodes, num_steps, dt, obs, drop_loads=False, step="fct"):
    cm = _common(asm)
    P = nonlinear_params()
    A = asm.convection(nonlinear_wind)
    Mat_p = -A - P["eps"] * cm.Ad
    mis = _Misfit(asm, cm.M, obs, dt, drop=drop_loads)
    pk[num_steps * nodes:] = _terminal(obs, uhat, uk, nodes, num_steps)
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        pk_np1 = pk[end:end + nodes]
        uk_n = uk[start:end]
        M_u2 = asm.weighted_mass(lambda at: at(uk_n) ** 2)
        Mat_rhs = M_u2 - cm.M
        rhs = _add(np.zeros(nodes), mis(i, uhat, uk, nodes))
        pk[start:end] = _fct(cm, -Mat_p, rhs, pk_np1, dt, step, non_flux_mat=Mat_rhs)
    return pk


def solve_adjoint_schnak_system(uk, vk, uhat, vhat, pk, qk, T, asm, nodes, num_steps, dt, obs, wind=None, wind_scale=None,
                                drop_loads=False, step="fct"):
    ou, ov = pair(obs)
    cm = _common(asm)
    P = schnak_params()
    Du, Dv, gamma, om1, om2 = P["Du"], P["Dv"], P["gamma"], P["omega1"], P["omega2"]
    mu, mv = _Misfit(asm, cm.M, ou, dt, drop=drop_loads), _Misfit(asm, cm.M, ov, dt, drop=drop_loads)
    pk[num_steps * nodes:] = _terminal(ou, uhat, uk, nodes, num_steps)
    qk[num_steps * nodes:] = _terminal(ov, vhat, vk, nodes, num_steps)
    A0 = asm.convection(wind or schnak_wind).T.tocsr()
    t = T
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        t -= dt
        A = A0 if wind_scale is None else float(wind_scale(t)) * A0
        q_np1 = qk[end:end + nodes]
        p_np1 = pk[end:end + nodes]
        u_n = uk[start:end]
        v_n = vk[start:end]
        M_u2 = asm.weighted_mass(lambda at: at(u_n) ** 2)
        rhs_q = _add(asm.load(lambda at: gamma * at(p_np1) * at(u_n) ** 2), mv(i, vhat, vk, nodes))
        Mat_q = cm.M + dt * (Dv * cm.Ad - om2 * A + gamma * M_u2)
        qk[start:end] = spsolve(Mat_q.tocsc(), cm.M @ q_np1 + dt * rhs_q)
        q_n = qk[start:end]
        Mat_p = Du * cm.Ad - om1 * A
        M_uv = asm.weighted_mass(lambda at: at(u_n) * at(v_n))
        rhs_p = _add(asm.load(lambda at: -2 * gamma * at(u_n) * at(v_n) * at(q_n)), mu(i, uhat, uk, nodes))
        Mat_rhs = gamma * cm.M - 2 * gamma * M_uv
        pk[start:end] = _fct(cm, Mat_p, rhs_p, p_np1, dt, step, non_flux_mat=Mat_rhs)
    return pk, qk


def solve_adjoint_chtxs_system(uk, vk, uhat, vhat, pk, qk, control, T, asm, nodes, num_steps, dt, obs, misfit="mass",
                               rescaling=1 / 10, growth=None, drop_loads=False, step="fct"):
    if misfit not in ("mass", "nodal"):
        raise ValueError(f"Invalid value for 'misfit': '{misfit}'. Must be one of ['mass', 'nodal'].")
    ou, ov = pair(obs)
    cm = _common(asm)
    P = chtxs_params()
    delta, Dm, Df, chi, eta = P["delta"], P["Dm"], P["Df"], P["chi"], P["eta"]
    mu = _Misfit(asm, cm.M, ou, dt, mass=misfit == "mass", drop=drop_loads)
    mv = _Misfit(asm, cm.M, ov, dt, mass=misfit == "mass", drop=drop_loads)
    pk[num_steps * nodes:] = _terminal(ou, uhat, uk, nodes, num_steps)
    qk[num_steps * nodes:] = _terminal(ov, vhat, vk, nodes, num_steps)
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
        rhs_p = _add(asm.load(lambda at: at(c_n) * at(q_np1) / rescaling), mu(i, uhat, uk, nodes))
        if growth is not None:
            rhs_p = rhs_p + asm.load(lambda at: go.dr(at(u_n), growth) * at(p_np1))
        pk[start:end] = _fct(cm, Mat_p, rhs_p, p_np1, dt, step)
        p_n = pk[start:end]
        rhs_q = _add(asm.chtxs_adjoint_rhs_q(u_n, p_n, chi, eta), mv(i, vhat, vk, nodes))
        qk[start:end] = spsolve(Mat_q, cm.M @ q_np1 + dt * rhs_q)
    return pk, qk


def cost(asm, M, uk, uhat, vk, vhat, ck, obs, nodes, num_steps, dt, beta):
    """the snapshot cost of the observed variables (vk / vhat None for the one-variable problem) and the control term"""
    ou, ov = pair(obs) if vk is not None else (obs, None)
    J = 0.0
    if ou is not None:
        J = J + so.misfit(asm, M, uk, uhat, ou, nodes)
    if ov is not None:
        J = J + so.misfit(asm, M, vk, vhat, ov, nodes)
    return J + beta / 2 * l2_norm_sq_Q(ck, num_steps, dt, M)


def chtxs_pgd_loop(asm, M, ic, targets, obs, num_steps, dt, growth, misfit="mass", beta=1e-3, c_lower=0.0, c_upper=20.0,
                   gam=1e-5, s0=2.0, rescaling=0.1, max_iter_armijo=20, iters=2):
    """The loop of ``oracle.pdeco.projected_gradient_descent("chtxs")`` (chemotaxis_FCT_PDECO_AT_refactored.py:112-290) for
    ``iters`` iterations without its fail / restart bookkeeping (the caller asserts that no search runs out of trials), with
    the per-step state sweep with growth, the snapshot adjoint and the snapshot cost.  Same history keys."""
    n, Nt = asm.n, num_steps
    tl = (Nt + 1) * n
    z = lambda x0: np.concatenate([np.asarray(x0, dtype=np.float64), np.zeros(Nt * n)])
    state = lambda c: tuple(a.copy() for a in go.solve_chtxs_system(c, z(ic[0]), z(ic[1]), asm, n, Nt, dt, rescaling=0.1,
                                                                    growth=growth, per_step=True))
    adjoint = lambda u, v, c: solve_adjoint_chtxs_system(u, v, targets[0], targets[1], np.zeros(tl), np.zeros(tl), c, Nt * dt,
                                                         asm, n, Nt, dt, obs, misfit=misfit, rescaling=rescaling, growth=growth)
    J = lambda u, v, c: cost(asm, M, u, targets[0], v, targets[1], c, obs, n, Nt, dt, beta)
    c = np.zeros(tl)
    u, v = state(c)
    p, q = adjoint(u, v, c)
    cost_old = J(u, v, c)
    hist = dict(cost=[cost_old], armijo_its=[], armijo_margin=[])
    for _ in range(iters):
        d = -(beta * c - q * u / rescaling)
        margins = []
        for k in range(max_iter_armijo):
            s = s0 / 2 ** k
            c_inc = np.clip(c + s * d, c_lower, c_upper)
            ut, vt = state(c_inc)
            Jk = J(ut, vt, c_inc)
            dif = l2_norm_sq_Q(c_inc - c, Nt, dt, M)
            margins.append((Jk - cost_old + gam / s * dif) / abs(cost_old))
            if Jk - cost_old <= -gam / s * dif:
                break
        c, u, v = c_inc, ut, vt
        p, q = adjoint(u, v, c)
        cost_old = J(u, v, c)
        hist["cost"].append(cost_old)
        hist["armijo_its"].append(k + 1)
        hist["armijo_margin"].append(margins)
    return dict(u=u, v=v, p=p, q=q, c=c, it=iters, **hist)
