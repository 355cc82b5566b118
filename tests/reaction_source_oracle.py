"""CPU reference of the linear source-control PDECO with an explicit (IMEX) reaction term
(``solvers.LinearReactionSourceControl``), built from the unchanged oracle: advection_FCT_PDECO_finaltime_exact.py:252-279
(state), :293-322 (adjoint), :344-370 (sensitivity).

    state / sensitivity   rhs_i = M src_i - Mg(g_{i-1}) u_{i-1},   u_i = FCT_alg(A_u, rhs_i, u_{i-1}),  A_u = Aa1 - eps Ad
    adjoint               rhs_i = -Mg(g_i) p_{i+1} [+ M (uhat_i - u_i) all-time],  p_i = FCT_alg(A_p, rhs_i, p_{i+1}),
                          A_p = -(Aa1 + Aa2) - eps Ad,  Aa2 = assemble(sigma_h u v dx)

Mg(g) = assemble(g_h u v dx) with g_h the P1 function of the nodal values (cubic integrand: the degree-5 rule of
``P1Assembler.weighted_mass`` is exact).  The projected-gradient loop is the one of source_control_oracle.py, run with
these sweeps in place of the reaction-free ones."""
import contextlib

import numpy as np

import source_control_oracle as sco
from oracle.assembly import P1Assembler, QUAD6_PTS, QUAD6_W
from oracle.mesh import SquareMesh
from oracle.traj import LinearSource, exact_velocity


# The device tabulates the wind at the 6 points of the degree-4 rule (Context.assemble_convection), the oracle's default
# is the 7-point degree-5 rule.  Both are exact for the polynomial winds (degree <= 3) of the other scripts; the wind of this
# study is sin * cos, for which the two rules differ by their quadrature error (1e-10 in a sweep at 21 x 21).  A reference
# that is to be compared with the device beyond that assembles the convection matrix with the device's rule.
DEVICE_WIND_RULE = (QUAD6_PTS, QUAD6_W)


class ReactionSource(LinearSource):
    """Matrices of the problem: ``g`` the coefficient trajectory, ``sigma`` the nodal field of Aa2 (None: Aa2 = 0)."""

    def __init__(self, asm, g, eps=1e-4, wind=exact_velocity, sigma=None, wind_rule=None):
        super().__init__(asm, eps=eps, wind=wind)
        self.g = np.asarray(g, dtype=np.float64)
        if wind_rule is not None:       # (points, weights): another quadrature of the convection matrix, see DEVICE_WIND_RULE
            self.A = asm.convection(wind, *wind_rule)
            self.A_u = self.A - eps * self.cm.Ad
            self.A_p = -self.A - eps * self.cm.Ad
        if sigma is not None:
            self.Aadj = self.A + self.wmass(sigma)
            self.A_p = -self.Aadj - eps * self.cm.Ad
        self._mg = {}

    def wmass(self, f):
        return self.asm.weighted_mass(lambda at: at(f))

    def Mg(self, level):
        """assemble(g_h u v dx) of the coefficient at a time level (kept: every sweep of a loop asks for the same ones)"""
        if level not in self._mg:
            n = self.asm.n
            self._mg[level] = self.wmass(self.g[level * n:(level + 1) * n])
        return self._mg[level]


def forward(rs, src, uk, nodes, num_steps, dt):
    """State sweep (level 0 of ``uk`` = initial condition); the sensitivity is the same with src = d and a zero level 0."""
    uk[nodes:] = np.zeros(num_steps * nodes)
    for i in range(1, num_steps + 1):
        start, end = i * nodes, (i + 1) * nodes
        u_n = uk[start - nodes:start]
        rhs = rs.cm.M @ src[start:end] - rs.Mg(i - 1) @ u_n
        uk[start:end] = rs.cm.fct(-rs.A_u, rhs, u_n, dt)
    return uk


def adjoint(rs, u, uhat, nodes, num_steps, dt, optim):
    p = np.zeros_like(u)
    if optim != "alltime":
        p[num_steps * nodes:] = uhat - u[num_steps * nodes:]
    for i in reversed(range(0, num_steps)):
        start, end = i * nodes, (i + 1) * nodes
        p_np1 = p[end:end + nodes]
        rhs = -(rs.Mg(i) @ p_np1)
        if optim == "alltime":
            rhs = rs.cm.M @ (uhat[start:end] - u[start:end]) + rhs
        p[start:end] = rs.cm.fct(-rs.A_p, rhs, p_np1, dt)
    return p


@contextlib.contextmanager
def _sweeps(fwd, adj):
    """source_control_oracle's loop looks its two sweeps up by name: hand it others for the duration of one call"""
    keep = sco.linear_forward, sco.adjoint
    sco.linear_forward, sco.adjoint = fwd, adj
    try:
        yield
    finally:
        sco.linear_forward, sco.adjoint = keep


def pgd_source_control(rs, u0, uhat, c0, beta, c_lower, c_upper, nodes, num_steps, dt, **kw):
    """The loop of ``source_control_oracle.pgd_source_control`` (same arguments and history) on the reaction problem."""
    with _sweeps(forward, adjoint):
        return sco.pgd_source_control(rs, u0, uhat, c0, beta, c_lower, c_upper, nodes, num_steps, dt, **kw)


def script_problem(nc, fields, wind, T=0.1):
    """The script's configuration on an nc x nc unit square (dx = 1/nc, dt = dx^2, round(T/dt) steps): the manufactured
    inputs ``fields(t, X, Y)`` (``solvers.finaltime_exact_fields``) as trajectories in FEniCS DoF order."""
    mesh = SquareMesh(0.0, 1.0, nc)
    dx = 1.0 / nc
    dt = dx ** 2
    Nt, n = round(T / dt), mesh.nodes
    grid = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
    X, Y = np.meshgrid(grid, grid)
    exact = lambda t: {k: np.asarray(v).reshape(-1) for k, v in fields(t, X, Y).items()}
    lev = [exact(i * dt) for i in range(Nt + 1)]
    F = {k: np.concatenate([f[k][mesh.dof_to_vertex] for f in lev]) for k in ("u", "p", "c", "g", "f")}
    return dict(mesh=mesh, n=n, Nt=Nt, dt=dt, dx=dx, F=F, exact=exact, u0=F["u"][:n].copy(),
                uhat_T=exact(T)["uhat"][mesh.dof_to_vertex], sigma=lev[0]["div"][mesh.dof_to_vertex], wind=wind)


def script_reference(prob, eps=1e-4):
    return ReactionSource(P1Assembler(prob["mesh"]), prob["F"]["g"], eps=eps, wind=prob["wind"], sigma=prob["sigma"],
                          wind_rule=DEVICE_WIND_RULE)
