"""CPU reference of the projected L-BFGS loops (``solvers.lbfgs_solidbody``, ``solvers.lbfgs_source_control``), a NumPy
loop over the unchanged oracle's pieces (oracle.traj sweeps and directions, oracle.fct cost and norm).

Inner products are the discrete L2(Q) ones of the cost, <a, b>_Q = dt sum_l w_l a_l^T M b_l with the trapezoid weights of
``l2_norm_sq_Q``; ``g`` is minus the loops' descent direction, the L2(Q) Riesz representative of the gradient.

The free set of a control c with gradient g: a value is bound iff (c <= lo and g > 0) or (c >= hi and g < 0).

The memory keeps up to ``memory`` pairs s_i = c_{k+1} - c_k, y_i = g_{k+1} - g_k; a pair is stored only if, unmasked,
<s, y>_Q > 1e-10 sqrt(<s, s>_Q <y, y>_Q).  A direction is the two-loop recursion on coefficient vectors over
F = [s_1..s_k, y_1..y_k, g], every inner product taken from the Gram matrix G of the fields masked to the free set: pair i
takes part iff G[s_i, y_i] > 0, rho_i = 1 / G[s_i, y_i], gamma = G[s, y] / G[y, y] of the newest pair that takes part (1 if
none does); dir = -(F r) on the free set and -g on the bound set.  If r^T G e_g <= 0 the ring is dropped and dir = -g.

An iteration: adjoint and g at (c, u = S(c), J); push the pair of the previous accepted step; dir; trials
c_t = clip(c + s0/2^t dir), the first with J(c_t) - J <= -gam/s_t ||c_t - c||^2_Q is accepted; if none is and the direction
was a quasi-Newton one, the ring is dropped and -g is searched in the same iteration; if that fails too the loop stops
with history["stalled"] = True.  There is no unconditional first step.  history["sweeps"] counts state and adjoint
sweeps cumulatively: the first state, then per iteration the adjoint and one state per trial looked at."""
import numpy as np

from oracle.fct import cost_functional, l2_norm_sq_Q

PAIR_TOL = 1e-10


def q_weights(num_steps):
    w = np.ones(num_steps + 1)
    w[0] = 0.5
    w[-1] = 0.5
    return w


def q_inner(a, b, num_steps, dt, M):
    A, B = np.asarray(a).reshape(num_steps + 1, -1), np.asarray(b).reshape(num_steps + 1, -1)
    w = q_weights(num_steps)
    return dt * sum(w[l] * (A[l] @ (M @ B[l])) for l in range(num_steps + 1))


def q_gram(fields, mask, num_steps, dt, M):
    """G[i, j] = <chi f_i, chi f_j>_Q (mask None: chi = 1)"""
    F = [np.asarray(f, dtype=np.float64) if mask is None else np.where(mask, f, 0.0) for f in fields]
    J = len(F)
    G = np.empty((J, J))
    for i in range(J):
        for j in range(i, J):
            G[i, j] = G[j, i] = q_inner(F[i], F[j], num_steps, dt, M)
    return G


def free_set(c, g, lo, hi):
    return ~(((c <= lo) & (g > 0)) | ((c >= hi) & (g < 0)))


def two_loop_coefficients(G, k):
    """r with H g = F r for F = [s_1..s_k, y_1..y_k, g] (oldest pair first) and the Gram matrix G of F; returns
    (r, number of pairs that take part)"""
    J = 2 * k + 1
    q = np.zeros(J)
    q[2 * k] = 1.0
    part = [i for i in range(k) if G[i, k + i] > 0]
    alpha = {}
    for i in reversed(part):
        alpha[i] = (G[i] @ q) / G[i, k + i]
        q[k + i] -= alpha[i]
    gamma = G[part[-1], k + part[-1]] / G[k + part[-1], k + part[-1]] if part else 1.0
    r = gamma * q
    for i in part:
        b = (G[k + i] @ r) / G[i, k + i]
        r[i] += alpha[i] - b
    return r, len(part)


def two_loop_vectors(S, Y, g, inner):
    """The textbook two-loop recursion on vectors, H g, with the same participation rule and scaling"""
    part = [i for i in range(len(S)) if inner(S[i], Y[i]) > 0]
    q = np.array(g, dtype=np.float64)
    alpha = {}
    for i in reversed(part):
        alpha[i] = inner(S[i], q) / inner(S[i], Y[i])
        q = q - alpha[i] * Y[i]
    if part:
        q = inner(S[part[-1]], Y[part[-1]]) / inner(Y[part[-1]], Y[part[-1]]) * q
    for i in part:
        b = inner(Y[i], q) / inner(S[i], Y[i])
        q = q + (alpha[i] - b) * S[i]
    return q


def combine(fields, coef, mask, fallback, fallback_scale):
    out = coef[0] * fields[0]
    for j in range(1, len(fields)):
        out = out + coef[j] * fields[j]
    return out if mask is None else np.where(mask, out, fallback_scale * fallback)


class LimitedMemory:
    def __init__(self, memory, num_steps, dt, M):
        self.memory, self.Nt, self.dt, self.M = int(memory), num_steps, dt, M
        self.S, self.Y = [], []

    def drop(self):
        self.S, self.Y = [], []

    def push(self, s, y):
        if self.memory < 1:
            return False
        G = q_gram([s, y], None, self.Nt, self.dt, self.M)
        if not G[0, 1] > PAIR_TOL * np.sqrt(G[0, 0] * G[1, 1]):
            return False
        self.S.append(s)
        self.Y.append(y)
        if len(self.S) > self.memory:
            del self.S[0], self.Y[0]
        return True

    def direction(self, c, g, lo, hi):
        """(dir, "qn" or "g", fraction of free values)"""
        mask = free_set(c, g, lo, hi)
        F = self.S + self.Y + [g]
        G = q_gram(F, mask, self.Nt, self.dt, self.M)
        r, used = two_loop_coefficients(G, len(self.S))
        if not r @ G[:, -1] > 0:
            self.drop()
            return -1.0 * g, "g", float(mask.mean())
        return combine(F, -r, mask, g, -1.0), ("qn" if used else "g"), float(mask.mean())


def lbfgs_loop(c0, state, cost, gradient, c_lower, c_upper, iters, num_steps, dt, M, memory=5, gam=1e-4, s0=1.0,
               max_armijo=10, tol=None):
    """state(c) -> u = S(c); cost(u, c) -> J; gradient(c, u) -> (p, g).  Returns (u, p, c, history)."""
    lm = LimitedMemory(memory, num_steps, dt, M)
    c = np.array(c0, dtype=np.float64)
    u = state(c)
    J = cost(u, c)
    sweeps = 1
    hist = dict(cost=[], armijo_k=[], armijo_margin=[], used=[], pairs=[], free_fraction=[], sweeps=[], rel_change=[],
                cost0=J, stalled=False)
    p = None
    c_old = g_old = None
    for _ in range(iters):
        p, g = gradient(c, u)
        sweeps += 1
        if c_old is not None:
            lm.push(1.0 * c + (-1.0) * c_old, 1.0 * g + (-1.0) * g_old)
        direction, used, free = lm.direction(c, g, c_lower, c_upper)
        pairs = len(lm.S)
        margins, found = [], None
        while found is None:
            for k in range(max_armijo):
                s = s0 * (1 / 2 ** k)
                ct = np.clip(c + s * direction, c_lower, c_upper)
                ut = state(ct)
                Jt = cost(ut, ct)
                sweeps += 1
                dist = l2_norm_sq_Q(ct - c, num_steps, dt, M)
                margins.append((Jt - J + gam / s * dist) / abs(J))
                if Jt - J <= -gam / s * dist:
                    found = k
                    break
            if found is None:
                if used != "qn":
                    break
                lm.drop()
                direction, used = -1.0 * g, "g"
        if found is None:
            hist["stalled"] = True
            break
        for key, v in (("cost", Jt), ("armijo_k", found + 1), ("armijo_margin", margins), ("used", used), ("pairs", pairs),
                       ("free_fraction", free), ("sweeps", sweeps), ("rel_change", abs(J - Jt) / abs(J))):
            hist[key].append(v)
        c_old, g_old = c, g
        c, u, J = ct, ut, Jt
        if tol is not None and hist["rel_change"][-1] < tol:
            break
    hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
    return u, p, c, hist


# ---------------------------------------------------------------------------------------------- solid-body drift control
def lbfgs_solidbody(sb, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, memory=5, gam=1e-4, s0=1.0,
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
    return lbfgs_loop(c0, state, cost, gradient, c_lower, c_upper, iters, Nt, dt, M, memory, gam, s0, max_armijo, tol)


def solidbody_case(beta, c_lower, c_upper, optim="alltime", nc=12, num_steps=20, dt=1e-2):
    """The issue's configurations: 13 x 13 nodes on [-1, 1]^2, 20 steps of 1e-2, u0 = exp(-15((x+0.2)^2+(y-0.1)^2)),
    om = pi/40, c0 = 1; all-time target = the trajectory of c = 2, final-time target = exp(-15((x+0.1)^2+(y-0.2)^2))."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    om = SquareMesh(-1, 1, nc)
    asm = P1Assembler(om)
    n = om.nodes
    tl = (num_steps + 1) * n
    sb = otraj.SolidBody(asm, om=np.pi / 40)
    u0 = np.exp(-15 * ((om.x + 0.2) ** 2 + (om.y - 0.1) ** 2))[om.dof_to_vertex]
    if optim == "alltime":
        uhat = np.zeros(tl)
        uhat[:n] = u0
        otraj.solidbody_forward(sb, 2.0 * np.ones(tl), uhat, n, num_steps, dt)
    else:
        uhat = np.exp(-15 * ((om.x + 0.1) ** 2 + (om.y - 0.2) ** 2))[om.dof_to_vertex]
    return dict(sb=sb, nc=nc, n=n, Nt=num_steps, dt=dt, tl=tl, u0=u0, uhat=uhat, c0=np.ones(tl), beta=beta, lo=c_lower,
                hi=c_upper, optim=optim, M=sb.cm.M)


CONFIGS = {"A": (1e-3, 0.0, 5.0, "alltime"), "B": (1e-4, 0.0, 2.5, "alltime"), "A-finaltime": (1e-3, 0.0, 5.0, "finaltime")}


def run_solidbody(cs, iters, memory, **kw):
    return lbfgs_solidbody(cs["sb"], cs["u0"], cs["uhat"], cs["c0"], cs["beta"], cs["lo"], cs["hi"], iters, cs["n"],
                           cs["Nt"], cs["dt"], memory=memory, optim=cs["optim"], **kw)


# ---------------------------------------------------------------------------------------------- linear source control
def lbfgs_source_control(ls, u0, uhat, c0, beta, c_lower, c_upper, iters, nodes, num_steps, dt, g=None, optim="alltime",
                         memory=5, gam=1e-4, s0=1.0, max_armijo=10, tol=None, starts=None, forward=None, adjoint=None):
    """gradient = beta c - p (minus the loop's d = -(beta c - p)); ``forward`` / ``adjoint``: the sweeps of a problem
    with a reaction term (reaction_source_oracle), default the linear ones"""
    from oracle.traj import linear_forward
    import control_intervals_oracle as cio
    import source_control_oracle as sco
    n, Nt, M = nodes, num_steps, ls.cm.M
    tl = (Nt + 1) * n
    src0 = np.zeros(tl) if g is None else np.asarray(g, dtype=np.float64)
    forward = linear_forward if forward is None else forward
    adjoint = sco.adjoint if adjoint is None else adjoint

    def state(c):
        u = np.zeros(tl)
        u[:n] = u0
        return forward(ls, src0 + c, u, n, Nt, dt)

    def gradient(c, u):
        p = adjoint(ls, u, uhat, n, Nt, dt, optim)
        d = -(beta * c - p)
        if starts is not None:
            d = cio.project(d, starts, Nt, n)
        return p, -1.0 * d

    cost = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim)
    return lbfgs_loop(c0, state, cost, gradient, c_lower, c_upper, iters, Nt, dt, M, memory, gam, s0, max_armijo, tol)


def source_case(nc=10, T=1.0):
    """The manufactured all-time problem of advection_FCT_PDECO_alltime_exact.py on nc x nc cells (source_control_oracle's
    test problem): dt = dx^2, the exact g, uhat and u0, beta = 1e-3, bounds [0, 0.5], c0 = 0"""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    mesh = SquareMesh(0.0, 1.0, nc)
    dx = 1.0 / nc
    dt = dx ** 2
    Nt, n = round(T / dt), mesh.nodes
    ax = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
    X, Y = np.meshgrid(ax, ax)
    f = [{k: v.reshape(-1) for k, v in otraj.exact_fields(i * dt, X, Y).items()} for i in range(Nt + 1)]
    F = {k: np.concatenate([fi[k][mesh.dof_to_vertex] for fi in f]) for k in ("u", "g", "uhat")}
    ls = otraj.LinearSource(P1Assembler(mesh), eps=1e-3)
    return dict(ls=ls, nc=nc, n=n, Nt=Nt, dt=dt, tl=(Nt + 1) * n, u0=F["u"][:n].copy(), uhat=F["uhat"], g=F["g"],
                c0=np.zeros((Nt + 1) * n), beta=1e-3, lo=0.0, hi=0.5, M=ls.cm.M)


def run_source(cs, iters, memory, **kw):
    return lbfgs_source_control(cs["ls"], cs["u0"], cs["uhat"], cs["c0"], cs["beta"], cs["lo"], cs["hi"], iters, cs["n"],
                                cs["Nt"], cs["dt"], g=cs["g"], optim="alltime", memory=memory, **kw)
