"""CPU reference of the initial-state recovery (``solvers.initial_state_solidbody``): given a fixed control trajectory c,
targets uhat, a background v_b and a box [lo, hi], minimise over the initial state v

    J(v) = T(u(v)) + beta0/2 (v - v_b)^T M (v - v_b),      u(v) = oracle.traj.solidbody_forward from u_0 = v under c,

a NumPy loop over the unchanged oracle: T = ``oracle.fct.cost_functional(u, uhat, c, beta=0, optim)`` (with ``obs`` the
snapshot misfit of snapshots_oracle.py), the adjoint p = ``oracle.traj.solidbody_adjoint`` (``snapshots_oracle.adjoint``)
of u(v), and the gradient g = beta0 (v - v_b) - p_0, the L2(Omega) representative (p(T) = uhat - u(T), so -p_0 stands for
the tracking term; no mass solve).  The adjoint is an FCT discretisation of the continuous adjoint, so g is inexact.

The iteration is ``lbfgs_oracle.lbfgs_loop``'s with the one-level inner product a^T M b in place of L2(Q): free set,
pair test (PAIR_TOL), two-loop recursion on Gram coefficients, the first trial v_t = clip(v + s0/2^t dir) with
J(v_t) - J <= -gam/s_t ||v_t - v||^2_M accepted, -g searched in the same iteration when no quasi-Newton trial passes,
``stalled`` when that fails too.  ``memory=0`` is projected gradient."""
import numpy as np

from oracle import traj as otraj
from oracle.fct import cost_functional

from lbfgs_oracle import PAIR_TOL, combine, free_set, two_loop_coefficients


def omega_inner(a, b, M):
    return a @ (M @ b)


def omega_gram(fields, mask, M):
    """G[i, j] = (chi f_i)^T M (chi f_j) (mask None: chi = 1)"""
    F = [np.asarray(f, dtype=np.float64) if mask is None else np.where(mask, f, 0.0) for f in fields]
    J = len(F)
    G = np.empty((J, J))
    for i in range(J):
        for j in range(i, J):
            G[i, j] = G[j, i] = omega_inner(F[i], F[j], M)
    return G


class LimitedMemory:
    """lbfgs_oracle.LimitedMemory with a^T M b"""

    def __init__(self, memory, M):
        self.memory, self.M = int(memory), M
        self.S, self.Y = [], []

    def drop(self):
        self.S, self.Y = [], []

    def push(self, s, y):
        if self.memory < 1:
            return False
        G = omega_gram([s, y], None, self.M)
        if not G[0, 1] > PAIR_TOL * np.sqrt(G[0, 0] * G[1, 1]):
            return False
        self.S.append(s)
        self.Y.append(y)
        if len(self.S) > self.memory:
            del self.S[0], self.Y[0]
        return True

    def coefficients(self, v, g, lo, hi):
        """(F, mask, G, r, pairs that took part) of the direction at v"""
        mask = free_set(v, g, lo, hi)
        F = self.S + self.Y + [g]
        G = omega_gram(F, mask, self.M)
        r, used = two_loop_coefficients(G, len(self.S))
        return F, mask, G, r, used

    def direction(self, v, g, lo, hi):
        """(dir, "qn" or "g", fraction of free values)"""
        F, mask, G, r, used = self.coefficients(v, g, lo, hi)
        if not r @ G[:, -1] > 0:
            self.drop()
            return -1.0 * g, "g", float(mask.mean())
        return combine(F, -r, mask, g, -1.0), ("qn" if used else "g"), float(mask.mean())


def initial_state_loop(v0, state, tracking, adjoint, vb, beta0, v_lower, v_upper, iters, M, memory=5, gam=1e-4, s0=1.0,
                       max_armijo=10, tol=None):
    """state(v) -> u; tracking(u) -> T; adjoint(u) -> p.  Returns (u, p, v, history): lbfgs_loop's history plus
    ``tracking`` and ``background``, the two terms of J at every accepted iterate."""
    lm = LimitedMemory(memory, M)
    v = np.array(v0, dtype=np.float64)
    n = v.size
    vb = np.zeros(n) if vb is None else np.asarray(vb, dtype=np.float64)

    def cost(u, vv):
        T = tracking(u)
        B = beta0 / 2 * omega_inner(vv - vb, vv - vb, M)
        return T + B, T, B

    u = state(v)
    J, T0, B0 = cost(u, v)
    sweeps = 1
    hist = dict(cost=[], armijo_k=[], armijo_margin=[], used=[], pairs=[], free_fraction=[], sweeps=[], rel_change=[],
                tracking=[], background=[], cost0=J, tracking0=T0, background0=B0, stalled=False)
    p = None
    v_old = g_old = None
    for _ in range(iters):
        p = adjoint(u)
        g = beta0 * (v - vb) - p[:n]
        sweeps += 1
        if v_old is not None:
            lm.push(1.0 * v + (-1.0) * v_old, 1.0 * g + (-1.0) * g_old)
        direction, used, free = lm.direction(v, g, v_lower, v_upper)
        pairs = len(lm.S)
        margins, found = [], None
        while found is None:
            for k in range(max_armijo):
                s = s0 * (1 / 2 ** k)
                vt = np.clip(v + s * direction, v_lower, v_upper)
                ut = state(vt)
                Jt, Tt, Bt = cost(ut, vt)
                sweeps += 1
                dist = omega_inner(vt - v, vt - v, M)
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
        for key, val in (("cost", Jt), ("armijo_k", found + 1), ("armijo_margin", margins), ("used", used),
                         ("pairs", pairs), ("free_fraction", free), ("sweeps", sweeps), ("rel_change", abs(J - Jt) / abs(J)),
                         ("tracking", Tt), ("background", Bt)):
            hist[key].append(val)
        v_old, g_old = v, g
        v, u, J = vt, ut, Jt
        if tol is not None and hist["rel_change"][-1] < tol:
            break
    hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
    return u, p, v, hist


def initial_state_solidbody(sb, c, uhat, v0, beta0, v_lower, v_upper, iters, nodes, num_steps, dt, background=None,
                            memory=5, gam=1e-4, s0=1.0, max_armijo=10, tol=None, optim="finaltime", obs=None):
    """``obs`` (anything with theta, tau, window, cost_w): snapshot tracking, ``uhat`` a trajectory; else the named mode"""
    n, Nt, M = nodes, num_steps, sb.cm.M
    tl = (Nt + 1) * n
    c = np.asarray(c, dtype=np.float64)
    uhat = np.asarray(uhat, dtype=np.float64)

    def state(v):
        u = np.zeros(tl)
        u[:n] = v
        return otraj.solidbody_forward(sb, c, u, n, Nt, dt)

    if obs is None:
        tracking = lambda u: cost_functional(u, uhat, c, Nt, dt, M, 0.0, optim)
        adjoint = lambda u: otraj.solidbody_adjoint(sb, c, u, uhat, np.zeros(tl), n, Nt, dt, optim=optim)
    else:
        import snapshots_oracle as so
        tracking = lambda u: so.misfit(sb.asm, M, u, uhat, obs, n)
        adjoint = lambda u: so.adjoint(sb, c, u, uhat, obs, n, Nt, dt)
    return initial_state_loop(v0, state, tracking, adjoint, background, beta0, v_lower, v_upper, iters, M, memory, gam, s0,
                              max_armijo, tol)


def case_i(nc=12, num_steps=20, dt=1e-2):
    """Case I: the mesh and sweep of ``ensemble_oracle.case_e`` (13 x 13 nodes on [-1, 1]^2, 20 steps of 1e-2, om = pi/40,
    eps = 0, drift (1, 1)), control c = 2, truth v* = exp(-15((x+0.2)^2 + (y-0.1)^2)), targets = the oracle's trajectory
    from v* (``traj``: its last level for final-time, all of it for all-time), start v0 = exp(-15((x-0.1)^2 + (y+0.2)^2)),
    background 0.5 v0, beta0 = 1e-3, box [0, 0.8]."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    om = SquareMesh(-1, 1, nc)
    asm = P1Assembler(om)
    n = om.nodes
    tl = (num_steps + 1) * n
    sb = otraj.SolidBody(asm, om=np.pi / 40)
    c = 2.0 * np.ones(tl)
    truth = np.exp(-15 * ((om.x + 0.2) ** 2 + (om.y - 0.1) ** 2))[om.dof_to_vertex]
    traj = np.zeros(tl)
    traj[:n] = truth
    otraj.solidbody_forward(sb, c, traj, n, num_steps, dt)
    v0 = np.exp(-15 * ((om.x - 0.1) ** 2 + (om.y + 0.2) ** 2))[om.dof_to_vertex]
    return dict(sb=sb, nc=nc, n=n, Nt=num_steps, dt=dt, tl=tl, c=c, truth=truth, traj=traj, v0=v0, vb=0.5 * v0, beta0=1e-3,
                lo=0.0, hi=0.8, M=sb.cm.M)


S0 = {"finaltime": 4.0, "alltime": 16.0}


def target(cs, optim):
    return cs["traj"] if optim != "finaltime" else cs["traj"][cs["Nt"] * cs["n"]:].copy()


def run(cs, optim, memory, iters=5, s0=None, obs=None, **kw):
    return initial_state_solidbody(cs["sb"], cs["c"], target(cs, optim), cs["v0"], cs["beta0"], cs["lo"], cs["hi"], iters,
                                   cs["n"], cs["Nt"], cs["dt"], background=cs["vb"], memory=memory,
                                   s0=S0[optim] if s0 is None else s0, optim=optim, obs=obs, **kw)
