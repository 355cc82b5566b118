"""CPU reference of the ensemble drift control (``solvers.ensemble_solidbody``): one control c for S scenarios with
initial conditions u0_s, targets uhat_s and weights pi_s >= 0 (normalised to sum 1),

    J(c) = sum_s pi_s T_s(u_s(c)) + beta/2 ||c||^2_Q,

a NumPy loop over the unchanged oracle: ``lbfgs_oracle.lbfgs_loop`` with three callbacks.  ``state(c)`` is S calls of
``oracle.traj.solidbody_forward``; the cost is sum_s pi_s cost_functional(u_s, uhat_s, c, beta=0) summed in index order
plus beta/2 l2_norm_sq_Q(c); the gradient is, per level,

    chebsi(-(beta M c_l + sum_s pi_s asm.drift_gradient(p_{s,l}, u_{s,l}, drift)), M, Md, 20, 0.5, 2)

projected with ``control_intervals_oracle.project`` when ``starts`` is given.  Every scenario has its own FCT adjoint
p_s = solidbody_adjoint(c, u_s, uhat_s): the limiter is nonlinear, so the weights are not folded into the adjoint loads.
A scenario of weight 0 enters neither sum."""
import numpy as np

from oracle import traj as otraj
from oracle.fct import chebsi, cost_functional, l2_norm_sq_Q

import lbfgs_oracle as lo


def normalise(weights, S):
    w = np.full(S, 1.0 / S) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.size == S and np.all(w >= 0) and np.all(np.isfinite(w)) and w.sum() > 0
    return w if weights is None else w / w.sum()


def first_equal(*rows):
    """rep[s] = the first scenario whose rows equal scenario s's bit for bit: a deterministic function is evaluated once
    per distinct scenario and copied (an ensemble of cycled scenarios costs what its distinct ones cost)"""
    seen, rep = {}, []
    for s in range(len(rows[0])):
        rep.append(seen.setdefault(tuple(r[s].tobytes() for r in rows), s))
    return rep


def states(sb, c, u0, n, Nt, dt):
    """(S, tl): the S forward sweeps under the one control"""
    tl = (Nt + 1) * n
    out = np.zeros((len(u0), tl))
    for s, r in enumerate(first_equal(u0)):
        if r < s:
            out[s] = out[r]
            continue
        out[s, :n] = u0[s]
        otraj.solidbody_forward(sb, c, out[s], n, Nt, dt)
    return out


def scenario_costs(sb, u, uhat, c, Nt, dt, optim):
    """T_s, the tracking term of every scenario"""
    T = np.empty(len(u))
    for s, r in enumerate(first_equal(u, uhat)):
        T[s] = T[r] if r < s else cost_functional(u[s], uhat[s], c, Nt, dt, sb.cm.M, 0.0, optim)
    return T


def weighted_sum(w, vals):
    """(w_a0 v_a0 + w_a1 v_a1) + ... over the non-zero weights, in index order"""
    acc = None
    for ws, v in zip(w, vals):
        if ws == 0:
            continue
        acc = ws * v if acc is None else acc + ws * v
    return acc


def cost(sb, u, uhat, c, w, beta, Nt, dt, optim):
    return weighted_sum(w, scenario_costs(sb, u, uhat, c, Nt, dt, optim)) + beta / 2 * l2_norm_sq_Q(c, Nt, dt, sb.cm.M)


def adjoints(sb, c, u, uhat, n, Nt, dt, optim):
    tl = (Nt + 1) * n
    out = np.empty((len(u), tl))
    for s, r in enumerate(first_equal(u, uhat)):
        out[s] = out[r] if r < s else otraj.solidbody_adjoint(sb, c, u[s], uhat[s], np.zeros(tl), n, Nt, dt, optim=optim)
    return out


def gradient_rhs(sb, c, u, p, w, beta, n, Nt):
    """-(beta M c_l + sum_s pi_s assemble(p_{s,l} (b.grad u_{s,l}) v dx)) for every level"""
    M = sb.cm.M
    out = np.empty((Nt + 1) * n)
    rep = first_equal(u, p)
    for l in range(Nt + 1):
        sl = slice(l * n, (l + 1) * n)
        G = {}
        for s in set(rep):
            G[s] = sb.asm.drift_gradient(p[s, sl], u[s, sl], sb.drift)
        acc = weighted_sum(w, [G[r] for r in rep])
        out[sl] = -(beta * (M @ c[sl]) + acc)
    return out


def direction(sb, c, u, p, w, beta, n, Nt, starts=None):
    M = sb.cm.M
    Md = M.diagonal()
    rhs = gradient_rhs(sb, c, u, p, w, beta, n, Nt)
    d = np.concatenate([chebsi(rhs[l * n:(l + 1) * n], M, Md, 20, 0.5, 2) for l in range(Nt + 1)])
    if starts is not None:
        import control_intervals_oracle as cio
        d = cio.project(d, starts, Nt, n)
    return d


def ensemble_solidbody(sb, u0, uhat, weights, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, memory=0, gam=1e-4,
                       s0=1.0, max_armijo=10, tol=None, optim="finaltime", starts=None):
    """Returns (u, p, c, history): u, p of shape (S, tl); history as ``lbfgs_oracle.lbfgs_loop`` plus ``scenario_costs``
    (T_s at every accepted iterate), ``worst`` and ``control_cost``."""
    n, Nt = nodes, num_steps
    u0 = np.asarray(u0, dtype=np.float64)
    uhat = np.asarray(uhat, dtype=np.float64)
    S = len(u0)
    w = normalise(weights, S)
    parts = {}          # cost value -> (T, control cost) of every trial looked at

    def state(c):
        return states(sb, c, u0, n, Nt, dt)

    def J(u, c):
        T = scenario_costs(sb, u, uhat, c, Nt, dt, optim)
        cc = beta / 2 * l2_norm_sq_Q(c, Nt, dt, sb.cm.M)
        val = weighted_sum(w, T) + cc
        parts[val] = (T, cc)
        return val

    def gradient(c, u):
        p = adjoints(sb, c, u, uhat, n, Nt, dt, optim)
        return p, -1.0 * direction(sb, c, u, p, w, beta, n, Nt, starts)

    u, p, c, hist = lo.lbfgs_loop(c0, state, J, gradient, c_lower, c_upper, iters, Nt, dt, sb.cm.M, memory, gam, s0,
                                  max_armijo, tol)
    hist["scenario_costs"] = [parts[v][0] for v in hist["cost"]]
    hist["worst"] = [float(T[w != 0].max()) for T in hist["scenario_costs"]]
    hist["control_cost"] = [parts[v][1] for v in hist["cost"]]
    return u, p, c, hist


def case_e(nc=12, num_steps=20, dt=1e-2, optim="finaltime", cycle=None):
    """Case E: 13 x 13 nodes on [-1, 1]^2, 20 steps of 1e-2, om = pi/40, eps = 0, drift (1, 1); three blobs
    exp(-15((x-a)^2 + (y-b)^2)) at (-0.2, 0.1), (0.1, -0.2), (0, 0.3); targets = the trajectories under the constant
    controls 1.5, 2.0, 2.5 (the last level for final-time); weights (0.5, 0.3, 0.2), beta = 1e-3, box [0, 5], c0 = 1.
    ``cycle``: S scenarios, the three cycled, with uniform weights."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    om = SquareMesh(-1, 1, nc)
    asm = P1Assembler(om)
    n = om.nodes
    tl = (num_steps + 1) * n
    sb = otraj.SolidBody(asm, om=np.pi / 40)
    centres = [(-0.2, 0.1), (0.1, -0.2), (0.0, 0.3)]
    u0 = np.stack([np.exp(-15 * ((om.x - a) ** 2 + (om.y - b) ** 2))[om.dof_to_vertex] for a, b in centres])
    traj = np.stack([states(sb, cv * np.ones(tl), u0[s:s + 1], n, num_steps, dt)[0] for s, cv in enumerate((1.5, 2.0, 2.5))])
    uhat = traj if optim == "alltime" else traj[:, num_steps * n:].copy()
    weights = np.array([0.5, 0.3, 0.2])
    if cycle is not None:
        pick = np.arange(cycle) % 3
        u0, uhat, weights = u0[pick], uhat[pick], None
    return dict(sb=sb, nc=nc, n=n, Nt=num_steps, dt=dt, tl=tl, u0=u0, uhat=uhat, weights=weights, c0=np.ones(tl),
                beta=1e-3, lo=0.0, hi=5.0, optim=optim, M=sb.cm.M)


def run(cs, iters, memory, s0=64.0, **kw):
    u, p, c, hist = ensemble_solidbody(cs["sb"], cs["u0"], cs["uhat"], cs["weights"], cs["c0"], cs["beta"], cs["lo"],
                                       cs["hi"], iters, cs["n"], cs["Nt"], cs["dt"], memory=memory, s0=s0,
                                       optim=cs["optim"], **kw)
    return u, p, c, hist
