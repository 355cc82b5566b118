"""CPU reference of state bounds as a Moreau-Yosida penalty (``solvers.StateBounds``) for the solid-body / linear family,
built from the unchanged oracle and the snapshot loop of snapshots_oracle.py:

    v_n = u_n - clip(u_n, lo, hi)                          the nodal violation, signed
    P(u) = gamma/2 sum_n sigma_n sum_i ml_i omega_i v_{n,i}^2,            J_gamma = J + P
    adjoint   p_Nt  gets  - sigma_Nt gamma omega .* v_Nt                   (nodal, like the tracking terminal condition)
              rhs_n gets  - (sigma_n/dt) gamma ml .* omega .* v_n          (sigma_0 = 0: level 0 is the fixed IC)

with the lumped mass ml.  ``adjoint`` is ``snapshots_oracle.adjoint`` statement for statement plus these two terms, so
bounds that nothing violates leave its bits (x - 0 = x).  ``bounds``: anything with ``gamma``, ``sigma(dt)``,
``nodal(nodes)`` and ``pairs(nodes, dt)`` (a ``solvers.StateBounds``), everything in FEniCS DoF order."""
import numpy as np

import snapshots_oracle as so
from oracle import traj as otraj
from oracle.assembly import row_lump_diag
from oracle.fct import l2_norm_sq_Q


def lumped(M):
    return np.asarray(row_lump_diag(M), dtype=np.float64).ravel()


def violation(u, lo, hi):
    """u - clip(u, lo, hi) written with min / max, the form that keeps a NaN in u"""
    c = u if lo is None else np.fmax(u, lo)
    c = c if hi is None else np.fmin(c, hi)
    return u - c


def stats(M, uk, bounds, nodes, dt):
    """``(P, max |v|, number of v != 0, that number / penalised pairs)`` over the pairs with sigma_n != 0, omega_i != 0"""
    lo, hi, w = bounds.nodal(nodes)
    ml, sigma = lumped(M), bounds.sigma(dt)
    on = np.ones(nodes, dtype=bool) if w is None else w != 0
    mw = ml if w is None else ml * w
    P, vmax, count = 0.0, 0.0, 0
    for lv in np.flatnonzero(sigma):
        v = violation(uk[lv * nodes:(lv + 1) * nodes], lo, hi)[on]
        P = P + sigma[lv] * np.sum(mw[on] * (v * v))
        vmax = max(vmax, np.abs(v).max()) if v.size else vmax
        count += int(np.count_nonzero(v))
    return 0.5 * bounds.gamma * P, vmax, count, count / max(1, bounds.pairs(nodes, dt))


def penalty(M, uk, bounds, nodes, dt):
    return stats(M, uk, bounds, nodes, dt)[0]


def adjoint(sb, ck, uk, uhat, obs, bounds, nodes, num_steps, dt, step="fct", Mg=None, A_p=None, interior=1.0):
    """``snapshots_oracle.adjoint`` with the penalty terms.  ``interior``: a factor on the interior penalty loads (the
    tests' broken variants: 0 drops them, -1 flips their sign)."""
    n, Nt = nodes, num_steps
    lo, hi, ws = bounds.nodal(n)
    ml, sigma, gamma = lumped(sb.cm.M), bounds.sigma(dt), bounds.gamma
    pk = np.zeros((Nt + 1) * n)
    w = obs.window
    if obs.tau != 0.0:
        d = uhat[Nt * n:] - uk[Nt * n:]
        pk[Nt * n:] = obs.tau * (d if w is None else w * d)
    sT = sigma[Nt] * gamma
    if sT != 0.0:                                   # (a level without a penalty is not read)
        pk[Nt * n:] = pk[Nt * n:] - (sT if ws is None else sT * ws) * violation(uk[Nt * n:], lo, hi)
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
                load = sb.asm.load(lambda at: at(uh_n) - at(u_n))
            else:
                load = sb.asm.load(lambda at: at(w) * (at(uh_n) - at(u_n)))
            rhs = (obs.theta[i] / dt) * load
        else:
            rhs = np.zeros(n)
        if Mg is not None:
            rhs = rhs - Mg(i) @ p_np1
        if (sigma[i] / dt) * gamma != 0.0:
            t = ((sigma[i] / dt) * gamma) * ml
            if ws is not None:
                t = t * ws
            rhs = rhs - interior * (t * violation(uk[start:end], lo, hi))
        pk[start:end] = so._step(sb, -A, rhs, p_np1, dt, step)
    return pk


def cost(sb, uk, uhat, ck, obs, bounds, nodes, num_steps, dt, beta):
    return so.cost(sb, uk, uhat, ck, obs, nodes, num_steps, dt, beta) + penalty(sb.cm.M, uk, bounds, nodes, dt)


def _record(hist, M, uk, bounds, n, dt):
    P, vmax, count, frac = stats(M, uk, bounds, n, dt)
    for key, v in (("penalty", P), ("max_violation", vmax), ("violated", count), ("violated_fraction", frac)):
        hist.setdefault(key, []).append(v)


def pgd_loop(sb, u0, uhat, obs, bounds, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, gam=1e-4, s0=1.0,
             max_armijo=10):
    """``snapshots_oracle.pgd_loop`` for J + P; the history gains the statistics of the accepted iterate."""
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
        pk = adjoint(sb, c_prev, uk, uhat, obs, bounds, n, Nt, dt)
        dk = otraj.solidbody_descent_direction(sb, c_prev, uk, pk, beta, n, Nt)
        ck = np.clip(c_prev + s0 * dk, c_lower, c_upper)
        otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
        J_k = cost(sb, uk, uhat, ck, obs, bounds, n, Nt, dt, beta)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            c_inc = np.clip(ck + s * dk, c_lower, c_upper)
            otraj.solidbody_forward(sb, c_inc, uk, n, Nt, dt)
            J = cost(sb, uk, uhat, c_inc, obs, bounds, n, Nt, dt, beta)
            stat = l2_norm_sq_Q(c_inc - ck, Nt, dt, sb.cm.M)
            margins.append((J - J_k + gam / s * stat) / abs(J_k))
            if not (J - J_k > -gam / s * stat):
                break
        hist["cost"].append(J)
        hist["armijo_k"].append(k + 1)
        hist["armijo_margin"].append(margins)
        _record(hist, sb.cm.M, uk, bounds, n, dt)
        c_prev = c_inc
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return uk, pk, c_prev, hist


def pgd_source_loop(ls, u0, uhat, obs, bounds, c0, beta, c_lower, c_upper, nodes, num_steps, dt, max_iters, gam=1e-4,
                    s0=1.0, max_armijo=10):
    """``source_control_oracle.pgd_source_control(increment="resolve")`` for J + P with the adjoint above on the fixed
    operator ``ls.A_p``, ``max_iters`` iterations (no stop test).  ``obs``: the mode as observations, ``uhat`` a trajectory."""
    n, Nt = nodes, num_steps
    tl = (Nt + 1) * n
    J_of = lambda u, c: cost(ls, u, uhat, c, obs, bounds, n, Nt, dt, beta)
    u = np.zeros(tl)
    u[:n] = u0
    c = np.array(c0, dtype=np.float64)
    J_ref = 10 * J_of(u, c)
    hist = dict(cost=[], cost_state=[], armijo_k=[], armijo_margin=[])
    p = np.zeros(tl)
    for _ in range(max_iters):
        otraj.linear_forward(ls, c, u, n, Nt, dt)
        hist["cost_state"].append(J_of(u, c))
        p = adjoint(ls, None, u, uhat, obs, bounds, n, Nt, dt, A_p=ls.A_p)
        d = -(beta * c - p)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            cj = np.clip(c + s * d, c_lower, c_upper)
            uj = np.zeros(tl)
            uj[:n] = u0
            otraj.linear_forward(ls, cj, uj, n, Nt, dt)
            Jj = J_of(uj, cj)
            dist = l2_norm_sq_Q(cj - c, Nt, dt, ls.cm.M)
            margins.append((Jj - J_ref + gam / s * dist) / abs(J_ref))
            if Jj - J_ref <= -gam / s * dist:
                break
        hist["cost"].append(Jj)
        hist["armijo_k"].append(k + 1)
        hist["armijo_margin"].append(margins)
        _record(hist, ls.cm.M, uj, bounds, n, dt)
        J_ref, c = Jj, cj
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return u, p, c, hist
