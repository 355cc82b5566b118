"""CPU reference of controls that are piecewise constant in time (``solvers.ControlIntervals``, ``control_time=``).

``starts``: K + 1 increasing integers, starts[0] = 0, starts[K] = num_steps + 1; interval k holds the levels
starts[k] <= l < starts[k+1].  With the trapezoid's level weights w_l = 1, w_0 = w_Nt = 1/2 (those of
``oracle.fct.l2_norm_sq_Q`` without dt) and W_k = sum_{l in k} w_l

    restrict(x)[k] = (sum_{l in k} w_l x_l) / W_k          prolong(y)[l] = y[k(l)]          project = prolong o restrict

the orthogonal projection in the L2(Q) inner product onto the controls constant on every interval.  The four
projected-gradient loops with the projection inserted behind their descent direction: the solid-body loops are the
oracle's with ``oracle.traj.solidbody_descent_direction`` wrapped (projected after its per-level ChebSI); the
source-control loop, which forms its direction inline, is source_control_oracle's restated around the ``oracle.traj``
sweeps; the loop of the three PDE systems is restated from ``oracle.pdeco.projected_gradient_descent`` the way
``systems_snapshots_oracle.chtxs_pgd_loop`` restates its own."""
import contextlib

import numpy as np

import chtxs_growth_oracle as go
import per_step_oracle as po
import snapshots_oracle as so
import source_control_oracle as sco
from oracle import traj as otraj
from oracle.fct import cost_functional, l2_norm_sq_Q


def check(starts, num_steps):
    st = np.asarray(starts, dtype=np.int64)
    assert st.ndim == 1 and st.size >= 2 and st[0] == 0 and st[-1] == num_steps + 1 and np.all(np.diff(st) > 0), starts
    return st


def level_weights(num_steps):
    w = np.ones(num_steps + 1)
    w[0] = w[num_steps] = 0.5
    return w


def restrict(x, starts, num_steps, nodes):
    """(K, nodes): the weighted means, summed level by level in level order"""
    st = check(starts, num_steps)
    x = np.asarray(x, dtype=np.float64).reshape(num_steps + 1, nodes)
    w = level_weights(num_steps)
    out = np.empty((st.size - 1, nodes))
    for k in range(st.size - 1):
        acc = w[st[k]] * x[st[k]]
        for l in range(st[k] + 1, st[k + 1]):
            acc = acc + w[l] * x[l]
        out[k] = acc / w[st[k]:st[k + 1]].sum()
    return out


def prolong(y, starts, num_steps):
    st = check(starts, num_steps)
    y = np.asarray(y, dtype=np.float64)
    return np.ascontiguousarray(np.repeat(y, np.diff(st), axis=0)).ravel()


def project(x, starts, num_steps, nodes):
    return prolong(restrict(x, starts, num_steps, nodes), starts, num_steps)


def deviation(c, starts, num_steps, nodes):
    """largest |c_l - c_{first level of l's interval}|: 0.0 for a control constant on the intervals"""
    st = check(starts, num_steps)
    x = np.asarray(c).reshape(num_steps + 1, nodes)
    return float(np.max(np.abs(x - np.repeat(x[st[:-1]], np.diff(st), axis=0))))


# ---------------------------------------------------------------------------------------------- solid-body drift control
@contextlib.contextmanager
def projected_direction(starts):
    """``oracle.traj.solidbody_descent_direction`` followed by the projection, for the duration of the block (the loops
    look the function up by name); None: nothing is replaced"""
    if starts is None:
        yield
        return
    keep = otraj.solidbody_descent_direction

    def direction(sb, ck, uk, pk, beta, nodes, num_steps):
        return project(keep(sb, ck, uk, pk, beta, nodes, num_steps), starts, num_steps, nodes)

    otraj.solidbody_descent_direction = direction
    try:
        yield
    finally:
        otraj.solidbody_descent_direction = keep


def solidbody_pgd_loop(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, starts, **kw):
    """``oracle.traj.solidbody_pgd_loop`` (same arguments and history) with the projected direction"""
    with projected_direction(starts):
        return otraj.solidbody_pgd_loop(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, **kw)


def solidbody_snapshots_pgd_loop(sb, u0, uhat, obs, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, starts, **kw):
    """``snapshots_oracle.pgd_loop`` with the projected direction"""
    with projected_direction(starts):
        return so.pgd_loop(sb, u0, uhat, obs, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, **kw)


# ---------------------------------------------------------------------------------------------- linear source control
def pgd_source_control(ls, u0, uhat, c0, beta, c_lower, c_upper, nodes, num_steps, dt, starts, g=None, optim="alltime",
                       increment="linear", gam=1e-4, s0=1.0, max_armijo=10, tol=1e-4, max_iters=1000, stop="both",
                       forward=None, adjoint=None):
    """``source_control_oracle.pgd_source_control``, statement for statement (same arguments and history), with
    d = project(-(beta c - p)) (``starts=None``: no projection); in linear mode the sensitivity is then S(project(d)).
    ``forward`` / ``adjoint``: the two sweeps (default: that module's ``linear_forward`` / ``adjoint``; reaction_source_oracle's
    for the problem with a reaction term)."""
    forward = sco.linear_forward if forward is None else forward
    adjoint = sco.adjoint if adjoint is None else adjoint
    n, Nt, M = nodes, num_steps, ls.cm.M
    tl = (Nt + 1) * n
    g = np.zeros(tl) if g is None else np.asarray(g, dtype=np.float64)
    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    u = np.zeros(tl)
    u[:n] = u0
    c = np.array(c0, dtype=np.float64)
    J_ref = 10 * cost(u, c)
    hist = dict(cost=[], cost_state=[], armijo_k=[], step=[], stop_crit=[], stop_crit2=[], armijo_margin=[])
    stop1 = stop2 = np.inf
    while ((stop2 >= tol) or (stop == "both" and stop1 >= tol)) and len(hist["cost"]) < max_iters:
        forward(ls, g + c, u, n, Nt, dt)
        hist["cost_state"].append(cost(u, c))
        p = adjoint(ls, u, uhat, n, Nt, dt, optim)
        d = -(beta * c - p)
        if starts is not None:
            d = project(d, starts, Nt, n)
        if increment == "linear":
            w = forward(ls, d, np.zeros(tl), n, Nt, dt)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            cj = np.clip(c + s * d, c_lower, c_upper)
            if increment == "linear":
                uj = u + s * w
            else:
                uj = np.zeros(tl)
                uj[:n] = u0
                forward(ls, g + cj, uj, n, Nt, dt)
            Jj = cost(uj, cj)
            dist = l2_norm_sq_Q(cj - c, Nt, dt, M)
            margins.append((Jj - J_ref + gam / s * dist) / abs(J_ref))
            if Jj - J_ref <= -gam / s * dist:
                break
        nc = l2_norm_sq_Q(c, Nt, dt, M)
        stop1 = dist / nc if nc > 0 else np.inf
        stop2 = abs(J_ref - Jj) / abs(J_ref)
        for key, v in (("cost", Jj), ("armijo_k", k + 1), ("step", s), ("stop_crit", stop1), ("stop_crit2", stop2),
                       ("armijo_margin", margins)):
            hist[key].append(v)
        J_ref, c = Jj, cj
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return u, p, c, hist


# ---------------------------------------------------------------------------------------------- the three PDE systems
SYSTEM_DEFAULTS = {      # oracle.pdeco.DEFAULTS' values that the loop below reads
    "nonlinear": dict(optim="finaltime", beta=1e-1, c_lower=-1.0, c_upper=1.0, max_iter_armijo=5, gam=1e-4, s0=1.0,
                      rescaling=1.0),
    "schnak": dict(optim="finaltime", beta=1e-1, c_lower=0.0, c_upper=10.0, max_iter_armijo=10, gam=1e-4, s0=1.0,
                   rescaling=1.0),
    "chtxs": dict(optim="alltime", beta=1e-3, c_lower=0.0, c_upper=20.0, max_iter_armijo=20, gam=1e-5, s0=2.0,
                  rescaling=0.1),
}


def systems_pgd_loop(problem, asm, M, ic, targets, num_steps, dt, starts, iters, per_step=False, growth=None, **overrides):
    """The loop of ``oracle.pdeco.projected_gradient_descent`` for ``iters`` iterations without its fail / restart
    bookkeeping (the caller asserts that no search runs out of trials), with d = project(pointwise expression) and, per
    ``per_step`` / ``growth``, the per-step sweeps of per_step_oracle.py and the growth sweeps of chtxs_growth_oracle.py.
    ``starts=None``: no projection.  Same history keys."""
    P = dict(SYSTEM_DEFAULTS[problem])
    P.update(overrides)
    optim, beta, r = P["optim"], P["beta"], P["rescaling"]
    n, Nt = ic[0].size, num_steps
    T, tl = Nt * dt, (Nt + 1) * n
    two = problem != "nonlinear"
    gamma = otraj.schnak_params()["gamma"]
    z = lambda x0: np.concatenate([np.asarray(x0, dtype=np.float64), np.zeros(Nt * n)])

    def state(c):
        if problem == "nonlinear":
            f = po.solve_nonlinear_equation if per_step else otraj.solve_nonlinear_equation
            return f(c, z(ic[0]), None, asm, n, Nt, dt)[0], None
        if problem == "schnak":
            f = po.solve_schnak_system if per_step else otraj.solve_schnak_system
            return f(c, z(ic[0]), z(ic[1]), asm, n, Nt, dt)
        return go.solve_chtxs_system(c, z(ic[0]), z(ic[1]), asm, n, Nt, dt, growth=growth, per_step=per_step)

    def adjoint(u, v, c):
        if problem == "nonlinear":
            if optim == "alltime":
                import nonlinear_alltime_oracle as nao
                return nao.solve_adjoint_nonlinear_equation(u, targets[0], np.zeros(tl), T, asm, n, Nt, dt), None
            return otraj.solve_adjoint_nonlinear_equation(u, targets[0], np.zeros(tl), T, asm, n, Nt, dt), None
        if problem == "schnak":
            return otraj.solve_adjoint_schnak_system(u, v, targets[0], targets[1], np.zeros(tl), np.zeros(tl), T, asm, n, Nt,
                                                     dt, None, optim)
        return go.solve_adjoint_chtxs_system(u, v, targets[0], targets[1], np.zeros(tl), np.zeros(tl), c, T, asm, n, Nt, dt,
                                             None, optim, rescaling=r, growth=growth)

    def J(u, v, c):
        if two:
            return cost_functional(u, targets[0], c, Nt, dt, M, beta, optim, var2=v, var2_target=targets[1])
        return cost_functional(u, targets[0], c, Nt, dt, M, beta, optim)

    c = np.zeros(tl)
    u, v = state(c)
    p, q = adjoint(u, v, c)
    cost_old = J(u, v, c)
    hist = dict(cost=[cost_old], armijo_its=[], armijo_margin=[])
    for _ in range(iters):
        if problem == "nonlinear":
            d = -(beta * c - p)
        elif problem == "schnak":
            d = -(beta * c - gamma / r * p)
        else:
            d = -(beta * c - q * u / r)
        if starts is not None:
            d = project(d, starts, Nt, n)
        margins = []
        for k in range(P["max_iter_armijo"]):
            s = P["s0"] / 2 ** k
            c_inc = np.clip(c + s * d, P["c_lower"], P["c_upper"])
            ut, vt = state(c_inc)
            Jk = J(ut, vt, c_inc)
            dif = l2_norm_sq_Q(c_inc - c, Nt, dt, M)
            margins.append((Jk - cost_old + P["gam"] / s * dif) / abs(cost_old))
            if Jk - cost_old <= -P["gam"] / s * dif:
                break
        c, u, v = c_inc, ut, vt
        p, q = adjoint(u, v, c)
        cost_old = J(u, v, c)
        hist["cost"].append(cost_old)
        hist["armijo_its"].append(k + 1)
        hist["armijo_margin"].append(margins)
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return dict(u=u, v=v, p=p, q=q, c=c, it=iters, **hist)
