"""CPU reference of the projected gradient descent of the linear source-control PDECO (``solvers.pgd_source_control``),
built from the unchanged oracle: advection_FCT_PDECO_alltime_exact.py:212-330 (all-time, stop on both criteria) and
advection_FCT_PDECO_finaltime.py:170-280 (final-time, stop on the cost only).

Per iteration: u = S(g + c_k) (IC kept), the adjoint (all-time: p(T) = 0, load M (uhat_n - u_n); final-time:
p(T) = uhat_T - u(T), no load), d = -(beta c_k - p), and an Armijo search over s_j = s0 / 2^j on c_j = clip(c_k + s_j d)
with J_j - J_ref <= -gam / s_j ||c_j - c_k||^2_Q.  increment="linear": J_j = J(u + s_j w, c_j) with the sensitivity
w = S(d) (zero IC, :282-297); increment="resolve": J_j = J(S(g + c_j), c_j).  J_ref starts at 10 J(u with level 0 only,
c_0) and is then the cost the previous iteration accepted."""
import numpy as np

from oracle.fct import cost_functional, l2_norm_sq_Q
from oracle.traj import linear_adjoint, linear_forward


def adjoint(ls, u, uhat, nodes, num_steps, dt, optim):
    if optim == "alltime":
        return linear_adjoint(ls, u, uhat, np.zeros_like(u), nodes, num_steps, dt)
    p = np.zeros_like(u)
    p[num_steps * nodes:] = uhat - u[num_steps * nodes:]
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        p[start:end] = ls.cm.fct(-ls.A_p, np.zeros(nodes), p[end:end + nodes], dt)
    return p


def pgd_source_control(ls, u0, uhat, c0, beta, c_lower, c_upper, nodes, num_steps, dt, g=None, optim="alltime",
                       increment="linear", gam=1e-4, s0=1.0, max_armijo=10, tol=1e-4, max_iters=1000, stop="both"):
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
        linear_forward(ls, g + c, u, n, Nt, dt)
        hist["cost_state"].append(cost(u, c))
        p = adjoint(ls, u, uhat, n, Nt, dt, optim)
        d = -(beta * c - p)
        if increment == "linear":
            w = linear_forward(ls, d, np.zeros(tl), n, Nt, dt)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            cj = np.clip(c + s * d, c_lower, c_upper)
            if increment == "linear":
                uj = u + s * w
            else:
                uj = np.zeros(tl)
                uj[:n] = u0
                linear_forward(ls, g + cj, uj, n, Nt, dt)
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
    return u, p, c, hist
