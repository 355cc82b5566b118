"""CPU checks of the reference loop of the linear source-control PDECO (source_control_oracle.py), config C1's
parameter set (advection_FCT_PDECO_alltime_exact.py: unit square, dt = dx^2, eps = 1e-3, beta = 1e-3, c in [0, 0.5]):
its gradient against a finite difference of the reduced cost, and the error table of the manufactured solution."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _problem(nc, T=1.0, dt=None):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    mesh = SquareMesh(0.0, 1.0, nc)
    dx = 1.0 / nc
    dt = dx ** 2 if dt is None else dt
    Nt, n = round(T / dt), mesh.nodes
    g = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
    X, Y = np.meshgrid(g, g)
    exact = lambda t: {k: v.reshape(-1) for k, v in otraj.exact_fields(t, X, Y).items()}
    f = [exact(i * dt) for i in range(Nt + 1)]
    F = {k: np.concatenate([fi[k][mesh.dof_to_vertex] for fi in f]) for k in ("u", "p", "c", "g", "uhat")}
    return mesh, otraj.LinearSource(P1Assembler(mesh), eps=1e-3), n, Nt, dt, dx, F, exact


def test_gradient_matches_finite_difference_of_reduced_cost():
    """<beta c - p, delta>_Q against (Jr(c + h delta) - Jr(c - h delta)) / 2h, Jr(c) = J(S(g + c), c), in a smooth
    direction that vanishes on the boundary.  The discrete adjoint of the FCT sweep is the gradient only to O(dt)
    (measured: 0.9 % at dt = 1e-2, 0.1 % at 5e-3)."""
    import source_control_oracle as sco
    from oracle.fct import cost_functional, l2_norm_sq_Q
    from oracle.traj import linear_forward
    for dt in (1e-2, 5e-3):
        mesh, ls, n, Nt, dt, dx, F, _ = _problem(10, T=0.25, dt=dt)
        M = ls.cm.M
        rng = np.random.default_rng(1)
        c = 0.25 + 0.1 * rng.standard_normal((Nt + 1) * n)
        x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
        bump = np.sin(np.pi * x) * np.sin(np.pi * y)
        delta = np.concatenate([bump * (0.5 + rng.random()) for _ in range(Nt + 1)])

        def reduced(cc):
            u = np.zeros((Nt + 1) * n)
            u[:n] = F["u"][:n]
            linear_forward(ls, F["g"] + cc, u, n, Nt, dt)
            return cost_functional(u, F["uhat"], cc, Nt, dt, M, 1e-3, "alltime"), u

        _, u = reduced(c)
        p = sco.adjoint(ls, u, F["uhat"], n, Nt, dt, "alltime")
        grad = 1e-3 * c - p
        ip = (l2_norm_sq_Q(grad + delta, Nt, dt, M) - l2_norm_sq_Q(grad - delta, Nt, dt, M)) / 4
        h = 1e-3
        fd = (reduced(c + h * delta)[0] - reduced(c - h * delta)[0]) / (2 * h)
        assert abs(ip - fd) < 0.02 * abs(fd), (dt, ip, fd)


def test_error_table_of_the_exact_control():
    """u = S(g + c_ex), p its all-time adjoint: the table's relative errors are the per-level maxima of the 1.0 % / 3.6 %
    that test_gpu_linear.py measures over the whole trajectory; the exact control has zero error."""
    import source_control_oracle as sco
    from oracle.traj import linear_forward
    hp = importlib.import_module("fem-fct-pdeco_amd")
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    mesh, ls, n, Nt, dt, dx, F, exact = _problem(10)
    u = np.zeros((Nt + 1) * n)
    u[:n] = F["u"][:n]
    linear_forward(ls, F["g"] + F["c"], u, n, Nt, dt)
    p = sco.adjoint(ls, u, F["uhat"], n, Nt, dt, "alltime")
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert abs(rel(u, F["u"]) - 0.010) < 5e-4 and abs(rel(p, F["p"]) - 0.036) < 5e-4
    e = solvers.source_control_errors(hp.SquareMeshP1(0.0, 1.0, 10), u, F["c"], p, exact, dx, dt, iterations=7)
    assert e["rel_c"] == 0.0 and e["werr_c"] == 0.0
    assert 0.010 <= e["rel_u"] < 0.02 and 0.036 <= e["rel_p"] < 0.06      # measured 1.53 % / 4.57 %
    # the "one step behind" convention: u at level i + 1, p at level i
    i = int(np.argmax([np.linalg.norm(exact((i + 1) * dt)["u"] - u[(i + 1) * n:(i + 2) * n][mesh.vertex_to_dof])
                       for i in range(Nt)]))
    assert np.isclose(e["werr_u"], dx * np.linalg.norm(exact((i + 1) * dt)["u"]
                                                       - u[(i + 1) * n:(i + 2) * n][mesh.vertex_to_dof]))
    fields = e["csv"].split(" , ")
    assert len(fields) == 7 and fields[-1] == "7" and float(fields[0]) == e["rel_u"]


def test_oracle_loop_first_iterations():
    """Both increment modes start from c = 0 with full steps (the script's behaviour: step 1 is accepted), the cost
    falls, and ||c_0|| = 0 makes the first stop_crit infinite."""
    import source_control_oracle as sco
    mesh, ls, n, Nt, dt, dx, F, _ = _problem(10, T=0.2)
    for inc in ("linear", "resolve"):
        u, p, c, h = sco.pgd_source_control(ls, F["u"][:n], F["uhat"], np.zeros((Nt + 1) * n), 1e-3, 0.0, 0.5, n, Nt,
                                            dt, g=F["g"], increment=inc, max_iters=3)
        assert h["armijo_k"] == [1, 1, 1] and np.isinf(h["stop_crit"][0])
        assert h["cost"][2] < h["cost"][1] < h["cost"][0] and c.max() <= 0.5 and c.min() >= 0.0
