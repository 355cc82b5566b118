#!/usr/bin/env python3
"""The final-time manufactured-solution study of the linear source-control PDECO with a reaction term,
advection_FCT_PDECO_finaltime_exact.py, on the MI355X backend: du/dt - eps lap u + div(w u) + g u = c + f on the unit
square, dt = dx^2, T = 0.1, eps = 1e-4, beta = 0.1, c in [0, 1], g explicit (IMEX).  Projected gradient descent from
c = 0 with the script's linear increment and its stop test on the cost; the script's own run is 4 iterations at dx = 0.05
(40 steps), --converge runs until the criterion falls below tol = 1e-4.  Prints the error line of
advection_FCT_PDECO_alltime_exact.py:440 (max relative errors of u, c, p, max dx-weighted errors, iterations).

Aa2 of the adjoint operator is assembled from the nodal values of the analytic div(w) (the script projects div(w) onto
cellwise constants).

usage: python examples/source_control_finaltime_exact_pdeco.py [--dx 0.05] [--converge] [--increment linear|resolve]"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--dx", type=float, nargs="+", default=[0.05])
ap.add_argument("--converge", action="store_true", help="run to tol = 1e-4 instead of the script's 4 iterations")
ap.add_argument("--increment", default="linear", choices=["linear", "resolve"])
args = ap.parse_args()

T, eps, beta, c_lower, c_upper = 0.1, 1e-4, 0.1, 0.0, 1.0
wind = solvers.finaltime_exact_wind()

for dx in args.dx:
    nc = round(1.0 / dx)
    V = hp.SquareMeshP1(0.0, 1.0, nc)
    n, dt = V.nodes, dx ** 2
    Nt = round(T / dt)
    grid = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
    X, Y = np.meshgrid(grid, grid)
    exact = lambda t: {k: v.ravel() for k, v in solvers.finaltime_exact_fields(t, X, Y).items()}
    fields = [exact(i * dt) for i in range(Nt + 1)]
    dof = lambda key: hp.reorder_vector_to_dof_time(np.concatenate([f[key] for f in fields]), Nt + 1, n, V.vertex_to_dof)
    one = lambda a: hp.reorder_vector_to_dof_time(a, 1, n, V.vertex_to_dof)
    prob = solvers.LinearReactionSourceControl(V, Nt, dt, wind, dof("g"), eps=eps, adjoint_mass=one(fields[0]["div"]))
    try:
        t0 = time.perf_counter()
        u, p, c, hist = solvers.pgd_source_control(prob, dof("u")[:n], one(exact(T)["uhat"]), np.zeros((Nt + 1) * n), beta,
                                                   c_lower, c_upper, g=dof("f"), optim="finaltime", stop="cost",
                                                   increment=args.increment, tol=1e-4,
                                                   max_iters=1000 if args.converge else 4)
        el = time.perf_counter() - t0
    finally:
        prob.close()
    err = solvers.source_control_errors(V, u, c, p, exact, dx, dt, hist["iterations"])
    print(f"dx={dx}, dt={dt:g}, T={T}, beta={beta}: {hist['iterations']} iterations in {el:.2f} s, "
          f"J_acc {hist['cost'][-1]:.4e}, re-solved J {hist['cost_state'][-1]:.4e}, armijo_k {hist['armijo_k']}")
    print(err["csv"])
