"""CPU reference of the proximal-gradient loops for L1-sparse controls (``solvers.prox_solidbody``,
``solvers.prox_source_control``), a NumPy loop over the unchanged oracle's pieces (oracle.traj sweeps and directions,
oracle.fct cost and norm) beside lbfgs_oracle.py, whose cases, weights and gradients it reuses.

The cost is F(c) = J(S(c), c) + alpha ||c||_{1,h} with the nodal-quadrature L1 norm
    ||c||_{1,h} = dt sum_l w_l sum_i ml_i |c_{l,i}|        (w_l the trapezoid weights of l2_norm_sq_Q, ml the lumped mass)
whose prox is pointwise.  The trial control for step s and direction d (the loops pass d = -g):
    x = c + s d, tau = s alpha, t = |x| - tau, v = copysign(t, x) if t > 0 else 0.0, prox = min(max(v, lo), hi)

An iteration at (c, u = S(c), F): adjoint and g; the residual ||prox(c - g; tau = alpha) - c||^2_Q; trials
c_t = prox(c - s_t g; s_t alpha), s_t = s0 / 2^t; the first with F(c_t) - F <= -gam/s_t ||c_t - c||^2_Q is accepted; if none
is the loop stops with history["stalled"] = True.  No unconditional first step.  history["sweeps"] counts as
lbfgs_oracle.lbfgs_loop does, and as there the history's lists have one entry per accepted step: a stalled iteration
leaves none."""
import numpy as np

from oracle.fct import cost_functional, l2_norm_sq_Q

import lbfgs_oracle as lo


def prox(x, tau, lo_, hi_):
    """clip(soft_threshold(x, tau), lo, hi): in one dimension the exact prox of tau |.| + the indicator of [lo, hi]"""
    x = np.asarray(x, dtype=np.float64)
    t = np.abs(x) - tau
    v = np.where(t > 0, np.copysign(t, x), 0.0)
    return np.minimum(np.maximum(v, lo_), hi_)


def prox_trial(c, s, d, alpha, lo_, hi_):
    return prox(c + s * d, s * alpha, lo_, hi_)


def lumped_mass(M):
    from oracle.assembly import row_lump_diag
    return np.asarray(row_lump_diag(M), dtype=np.float64).ravel()


def l1_norm_Q(c, num_steps, dt, ml):
    C = np.abs(np.asarray(c, dtype=np.float64).reshape(num_steps + 1, -1))
    w = lo.q_weights(num_steps)
    return dt * sum(w[l] * (ml @ C[l]) for l in range(num_steps + 1))


def prox_loop(c0, state, cost, gradient, alpha, c_lower, c_upper, iters, num_steps, dt, M, gam=1e-4, s0=1.0, max_armijo=10,
              tol=None):
    """state(c) -> u = S(c); cost(u, c) -> J; gradient(c, u) -> (p, g).  Returns (u, p, c, history)."""
    ml = lumped_mass(M)
    c = np.array(c0, dtype=np.float64)
    u = state(c)
    J = cost(u, c)
    l1 = l1_norm_Q(c, num_steps, dt, ml)
    F = J + alpha * l1
    sweeps = 1
    hist = dict(cost=[], cost_smooth=[], l1=[], nonzero_fraction=[], residual=[], armijo_k=[], step=[], armijo_margin=[],
                rel_change=[], sweeps=[], cost0=F, stalled=False)
    p = None
    for _ in range(iters):
        p, g = gradient(c, u)
        sweeps += 1
        d = -1.0 * g
        r = prox_trial(c, 1.0, d, alpha, c_lower, c_upper)
        residual = l2_norm_sq_Q(r - c, num_steps, dt, M)
        margins, found = [], None
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            ct = prox_trial(c, s, d, alpha, c_lower, c_upper)
            ut = state(ct)
            Jt = cost(ut, ct)
            l1t = l1_norm_Q(ct, num_steps, dt, ml)
            Ft = Jt + alpha * l1t
            sweeps += 1
            dist = l2_norm_sq_Q(ct - c, num_steps, dt, M)
            margins.append((Ft - F + gam / s * dist) / abs(F))
            if Ft - F <= -gam / s * dist:
                found = k
                break
        if found is None:
            hist["stalled"] = True
            break
        for key, v in (("cost", Ft), ("cost_smooth", Jt), ("l1", l1t), ("nonzero_fraction", float(np.mean(ct != 0))),
                       ("residual", residual), ("armijo_k", found + 1), ("step", s), ("armijo_margin", margins),
                       ("rel_change", abs(F - Ft) / abs(F)), ("sweeps", sweeps)):
            hist[key].append(v)
        c, u, F = ct, ut, Ft
        if tol is not None and hist["rel_change"][-1] < tol:
            break
    hist["iterations"] = len(hist["cost"])
    hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
    return u, p, c, hist


# ---------------------------------------------------------------------------------------------- solid-body drift control
def prox_solidbody(sb, u0, uhat, c0, beta, alpha, c_lower, c_upper, iters, nodes, num_steps, dt, gam=1e-4, s0=1.0,
                   max_armijo=10, tol=None, optim="finaltime", starts=None):
    """``starts``: interval boundaries of a piecewise-constant control (the direction is projected), or None"""
    from oracle import traj as otraj
    import control_intervals_oracle as cio
    n, Nt, M = nodes, num_steps, sb.cm.M
    tl = (Nt + 1) * n
    uhat = np.asarray(uhat, dtype=np.float64)

    def state(c):
        u = np.zeros(tl)
        u[:n] = u0
        return otraj.solidbody_forward(sb, c, u, n, Nt, dt)

    def gradient(c, u):
        p = otraj.solidbody_adjoint(sb, c, u, uhat, np.zeros(tl), n, Nt, dt, optim=optim)
        d = otraj.solidbody_descent_direction(sb, c, u, p, beta, n, Nt)
        if starts is not None:
            d = cio.project(d, starts, Nt, n)
        return p, -1.0 * d

    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    return prox_loop(c0, state, cost, gradient, alpha, c_lower, c_upper, iters, Nt, dt, M, gam, s0, max_armijo, tol)


def run_solidbody(cs, iters, alpha, **kw):
    return prox_solidbody(cs["sb"], cs["u0"], cs["uhat"], cs["c0"], cs["beta"], alpha, cs["lo"], cs["hi"], iters, cs["n"],
                          cs["Nt"], cs["dt"], optim=cs["optim"], **kw)


DRIFT_S0, DRIFT_ITERS = 256.0, 8
DRIFT_ARMIJO_K = {1e-4: [1, 3, 1, 4, 1, 2, 3, 2], 5e-4: [1, 3, 1, 4, 1, 1, 2, 3]}


def drift_case():
    """13 x 13 nodes, 20 steps, beta = 1e-4, box [-1, 2.5], all-time; the target is the trajectory of the control that is
    2 on levels 0..10 and 0 after; c0 = 0"""
    from oracle import traj as otraj
    cs = lo.solidbody_case(1e-4, -1.0, 2.5, "alltime")
    n, Nt, tl = cs["n"], cs["Nt"], cs["tl"]
    ctrue = np.zeros(tl)
    ctrue[:11 * n] = 2.0
    uhat = np.zeros(tl)
    uhat[:n] = cs["u0"]
    otraj.solidbody_forward(cs["sb"], ctrue, uhat, n, Nt, cs["dt"])
    cs.update(uhat=uhat, c0=np.zeros(tl))
    return cs


# ---------------------------------------------------------------------------------------------- linear source control
def prox_source_control(ls, u0, uhat, c0, beta, alpha, c_lower, c_upper, iters, nodes, num_steps, dt, g=None,
                        optim="alltime", gam=1e-4, s0=1.0, max_armijo=10, tol=None, starts=None):
    from oracle.traj import linear_forward
    import control_intervals_oracle as cio
    import source_control_oracle as sco
    n, Nt, M = nodes, num_steps, ls.cm.M
    tl = (Nt + 1) * n
    src0 = np.zeros(tl) if g is None else np.asarray(g, dtype=np.float64)

    def state(c):
        u = np.zeros(tl)
        u[:n] = u0
        return linear_forward(ls, src0 + c, u, n, Nt, dt)

    def gradient(c, u):
        p = sco.adjoint(ls, u, uhat, n, Nt, dt, optim)
        d = -(beta * c - p)
        if starts is not None:
            d = cio.project(d, starts, Nt, n)
        return p, -1.0 * d

    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    return prox_loop(c0, state, cost, gradient, alpha, c_lower, c_upper, iters, Nt, dt, M, gam, s0, max_armijo, tol)


# (alpha, s0, iterations) -> armijo_k
SOURCE_RUNS = {(1e-2, 1024.0, 8): [1, 3, 1, 3, 1, 3, 1, 4], (3e-3, 64.0, 6): [1, 1, 1, 2, 2, 3]}


def source_case():
    """lbfgs_oracle.source_case(nc=6, T=0.5): n = 49, 18 steps, dt = 1/36; box [-0.1, 0.5];
    c0 = 0.08 cos(3 pi x) cos(2 pi y) at every level, in DoF order"""
    from oracle.mesh import SquareMesh
    cs = lo.source_case(nc=6, T=0.5)
    mesh = SquareMesh(0.0, 1.0, cs["nc"])
    c0 = (0.08 * np.cos(3 * np.pi * mesh.x) * np.cos(2 * np.pi * mesh.y))[mesh.dof_to_vertex]
    cs.update(lo=-0.1, hi=0.5, c0=np.tile(c0, cs["Nt"] + 1))
    return cs


def run_source(cs, iters, alpha, s0, **kw):
    return prox_source_control(cs["ls"], cs["u0"], cs["uhat"], cs["c0"], cs["beta"], alpha, cs["lo"], cs["hi"], iters,
                               cs["n"], cs["Nt"], cs["dt"], g=cs["g"], optim="alltime", s0=s0, **kw)
