"""CPU reference of controls that are piecewise constant in space (``solvers.ControlZones``, ``control_space=``), from the
dense indicator matrix chi (n x m, chi[i, j] = 1 when node i carries label j; a node labelled -1 has a zero row):

    restrict(x)     = chi^T x   (``M`` given: chi^T M x)          gram = chi^T M chi  (m x m, SPD)
    prolong(s)      = chi s     (``Ginv`` given: chi Ginv s)       project(x) = chi G^-1 chi^T M x

project is the orthogonal projection in the mass inner product onto span{chi_j}; for a dual right-hand side r the
steepest-descent direction among zone-constant controls is ``direction(r) = chi G^-1 chi^T r``, without a mass solve.

The loops: the solid-body ones are the oracle's with ``oracle.traj.solidbody_descent_direction`` replaced for their
duration by chi G^-1 chi^T rhs built from ``oracle.traj.solidbody_descent_rhs`` (no Chebyshev solve, like the device);
the source-control loop is control_intervals_oracle's restated with a projection callable; the L-BFGS loops hand a
projected gradient to ``lbfgs_oracle.lbfgs_loop``.  ``starts`` (interval boundaries of ``control_time=``) composes: time
restriction, the zone operation on the K fields, time prolongation."""
import contextlib

import numpy as np

import control_intervals_oracle as cio
import lbfgs_oracle as lo
import source_control_oracle as sco
from oracle import traj as otraj
from oracle.fct import chebsi, cost_functional, l2_norm_sq_Q


def check(labels, m):
    lab = np.asarray(labels, dtype=np.int64)
    assert lab.ndim == 1 and lab.min() >= -1 and lab.max() == m - 1 and 1 <= m <= 256, (m, lab.min(), lab.max())
    assert np.all(np.bincount(lab[lab >= 0], minlength=m) > 0)
    return lab


def chi(labels, m):
    lab = check(labels, m)
    X = np.zeros((lab.size, m))
    act = np.flatnonzero(lab >= 0)
    X[act, lab[act]] = 1.0
    return X


def restrict(x, labels, m, M=None):
    """(fields, m): chi^T x_f, or chi^T (M x_f)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, len(labels))
    y = x if M is None else np.stack([M @ xf for xf in x])
    return y @ chi(labels, m)


def gram(labels, m, M):
    X = chi(labels, m)
    G = X.T @ (M @ X)
    return 0.5 * (G + G.T)


def prolong(s, labels, m, Ginv=None):
    """(fields, n): chi (Ginv s_f)"""
    s = np.asarray(s, dtype=np.float64).reshape(-1, m)
    d = s if Ginv is None else s @ np.asarray(Ginv).T
    return d @ chi(labels, m).T


def direction(r, labels, m, M):
    """chi G^-1 chi^T r for the dual fields r: (fields, n)"""
    return prolong(restrict(r, labels, m), labels, m, np.linalg.inv(gram(labels, m, M)))


def project(x, labels, m, M):
    """chi G^-1 chi^T M x for the primal fields x: (fields, n)"""
    return prolong(restrict(x, labels, m, M), labels, m, np.linalg.inv(gram(labels, m, M)))


def deviation(c, labels, m):
    """largest |c_i - c_{first node of i's zone}| over the labelled nodes and all levels: 0.0 for a zone-constant control"""
    lab = check(labels, m)
    x = np.asarray(c).reshape(-1, lab.size)
    first = np.array([np.argmax(lab == j) for j in range(m)])
    act = lab >= 0
    return float(np.max(np.abs(x[:, act] - x[:, first][:, lab[act]])))


def in_time(op, x, starts, num_steps, nodes):
    """op on the fields of a trajectory, or between the time restriction and prolongation of ``starts``"""
    if starts is None:
        return op(np.asarray(x).reshape(num_steps + 1, nodes)).ravel()
    return cio.prolong(op(cio.restrict(x, starts, num_steps, nodes)), starts, num_steps)


# ---------------------------------------------------------------------------------------------- solid-body drift control
def solidbody_rhs(sb, ck, uk, pk, beta, nodes, num_steps):
    return np.concatenate([otraj.solidbody_descent_rhs(sb, ck, uk, pk, beta, nodes, l) for l in range(num_steps + 1)])


def solidbody_direction(sb, ck, uk, pk, beta, nodes, num_steps, labels, m, starts=None, cheb=False, extra_rhs=None):
    """chi G^-1 chi^T rhs per level (``cheb``: P(ChebSI(rhs)), which differs by the Chebyshev truncation only);
    ``extra_rhs``: a trajectory added to the right-hand side (the smoothness term's)"""
    M = sb.cm.M
    rhs = solidbody_rhs(sb, ck, uk, pk, beta, nodes, num_steps)
    if extra_rhs is not None:
        rhs = rhs + extra_rhs
    if cheb:
        Md = M.diagonal()
        d = np.concatenate([chebsi(r, M, Md, 20, 0.5, 2) for r in rhs.reshape(num_steps + 1, nodes)])
        return in_time(lambda x: project(x, labels, m, M), d, starts, num_steps, nodes)
    return in_time(lambda x: direction(x, labels, m, M), rhs, starts, num_steps, nodes)


@contextlib.contextmanager
def zone_direction(labels, m, starts=None, cheb=False):
    """``oracle.traj.solidbody_descent_direction`` replaced by the zone direction for the duration of the block (the
    loops look the function up by name)"""
    keep = otraj.solidbody_descent_direction

    def replaced(sb, ck, uk, pk, beta, nodes, num_steps):
        return solidbody_direction(sb, ck, uk, pk, beta, nodes, num_steps, labels, m, starts, cheb)

    otraj.solidbody_descent_direction = replaced
    try:
        yield
    finally:
        otraj.solidbody_descent_direction = keep


def solidbody_pgd_loop(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, labels, m, starts=None,
                       cheb=False, **kw):
    """``oracle.traj.solidbody_pgd_loop`` (same arguments and history) with the zone direction"""
    with zone_direction(labels, m, starts, cheb):
        return otraj.solidbody_pgd_loop(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, **kw)


def solidbody_snapshots_pgd_loop(sb, u0, uhat, obs, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, labels, m,
                                 starts=None, **kw):
    """``snapshots_oracle.pgd_loop`` with the zone direction"""
    import snapshots_oracle as so
    with zone_direction(labels, m, starts):
        return so.pgd_loop(sb, u0, uhat, obs, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, **kw)


def lbfgs_solidbody(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, labels, m, starts=None, memory=5,
                    gam=1e-4, s0=1.0, max_armijo=10, tol=None, optim="finaltime"):
    """``lbfgs_oracle.lbfgs_solidbody`` with the gradient -(zone direction)"""
    n, Nt, M = nodes, num_steps, sb.cm.M
    tl = (Nt + 1) * n
    uhat = np.asarray(uhat, dtype=np.float64)

    def state(c):
        u = np.zeros(tl)
        u[:n] = u0
        return otraj.solidbody_forward(sb, c, u, n, Nt, dt)

    def gradient(c, u):
        p = otraj.solidbody_adjoint(sb, c, u, uhat, np.zeros(tl), n, Nt, dt, optim=optim)
        return p, -1.0 * solidbody_direction(sb, c, u, p, beta, n, Nt, labels, m, starts)

    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    return lo.lbfgs_loop(c0, state, cost, gradient, c_lower, c_upper, iters, Nt, dt, M, memory, gam, s0, max_armijo, tol)


# ---------------------------------------------------------------------------------------------- linear source control
def source_projection(M, labels, m, starts, num_steps, nodes):
    return lambda d: in_time(lambda x: project(x, labels, m, M), d, starts, num_steps, nodes)


def pgd_source_control(ls, u0, uhat, c0, beta, c_lower, c_upper, nodes, num_steps, dt, projection, g=None, optim="alltime",
                       increment="linear", gam=1e-4, s0=1.0, max_armijo=10, tol=1e-4, max_iters=1000, stop="both",
                       forward=None, adjoint=None):
    """``control_intervals_oracle.pgd_source_control``, statement for statement, with d = projection(-(beta c - p))
    (``projection=None``: none); in linear mode the sensitivity is then S(projection(d))."""
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
        if projection is not None:
            d = projection(d)
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


def lbfgs_source_control(ls, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, projection, g=None,
                         optim="alltime", memory=5, gam=1e-4, s0=1.0, max_armijo=10, tol=None, forward=None, adjoint=None):
    """``lbfgs_oracle.lbfgs_source_control`` with the gradient -projection(-(beta c - p))"""
    n, Nt, M = nodes, num_steps, ls.cm.M
    tl = (Nt + 1) * n
    src0 = np.zeros(tl) if g is None else np.asarray(g, dtype=np.float64)
    forward = otraj.linear_forward if forward is None else forward
    adjoint = sco.adjoint if adjoint is None else adjoint

    def state(c):
        u = np.zeros(tl)
        u[:n] = u0
        return forward(ls, src0 + c, u, n, Nt, dt)

    def gradient(c, u):
        p = adjoint(ls, u, uhat, n, Nt, dt, optim)
        return p, -1.0 * projection(-(beta * c - p))

    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    return lo.lbfgs_loop(c0, state, cost, gradient, c_lower, c_upper, iters, Nt, dt, M, memory, gam, s0, max_armijo, tol)
