#!/usr/bin/env python3
"""The manufactured-solution study of the linear source-control PDECO, advection_FCT_PDECO_alltime_exact.py, on the
MI355X backend: config C1's parameter set (unit square, dt = dx^2, T = 1, eps = 1e-3, beta = 1e-3, c in [0, 0.5]),
projected gradient descent from c = 0 with the scripts' linear increment, stopped when both criteria fall below tol = 1e-4
(at most 1000 iterations).  Prints the script's error line (max relative errors of u, c, p, max dx-weighted errors,
iterations; :440) for dx = 0.1 and 0.05.

usage: python examples/source_control_exact_pdeco.py [--dx 0.1 0.05] [--increment linear|resolve]"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--dx", type=float, nargs="+", default=[0.1, 0.05])
ap.add_argument("--increment", default="linear", choices=["linear", "resolve"])
args = ap.parse_args()

T, eps, beta, c_lower, c_upper, e1, e2 = 1.0, 1e-3, 1e-3, 0.0, 0.5, 0.2, 0.3


def velocity(x, y):
    """advection_FCT_PDECO_alltime_exact.py:132-135"""
    return 2 * (y - 0.5) * x * (1 - x), -2 * (x - 0.5) * y * (1 - y)


def exact(t, X, Y):
    """uex, pex, cex, gex, uhatex of advection_FCT_PDECO_alltime_exact.py:77-128 (k1 = k2 = 1)"""
    pi = np.pi
    sx, sy, cx, cy = np.sin(pi * X), np.sin(pi * Y), np.cos(pi * X), np.cos(pi * Y)
    u = np.exp(e1 * t) * (sx * sy) ** 2
    amp = np.exp(e2 * T) - np.exp(e2 * t)
    p = amp * (sx * sy) ** 2
    c = np.clip(p / beta, c_lower, c_upper)
    wx, wy = velocity(X, Y)
    lap_u = 2 * pi ** 2 * np.exp(e1 * t) * (np.cos(2 * pi * X) * sy ** 2 + sx ** 2 * np.cos(2 * pi * Y))
    g = e1 * u - eps * lap_u + wx * 2 * pi * np.exp(e1 * t) * sx * cx * sy ** 2 \
        + wy * 2 * pi * np.exp(e1 * t) * sx ** 2 * sy * cy - c
    lap_p = 2 * pi ** 2 * amp * (np.cos(2 * pi * X) * sy ** 2 + sx ** 2 * np.cos(2 * pi * Y))
    uhat = e2 * np.exp(e2 * t) * (sx * sy) ** 2 - eps * lap_p - wx * 2 * pi * amp * sx * cx * sy ** 2 \
        - wy * 2 * pi * amp * sx ** 2 * sy * cy + u
    return dict(u=u.ravel(), p=p.ravel(), c=c.ravel(), g=g.ravel(), uhat=uhat.ravel())


for dx in args.dx:
    nc = round(1.0 / dx)
    V = hp.SquareMeshP1(0.0, 1.0, nc)
    n, dt = V.nodes, dx ** 2
    Nt = round(T / dt)
    grid = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
    X, Y = np.meshgrid(grid, grid)
    fields = [exact(i * dt, X, Y) for i in range(Nt + 1)]
    dof = lambda key: hp.reorder_vector_to_dof_time(np.concatenate([f[key] for f in fields]), Nt + 1, n, V.vertex_to_dof)
    g, uhat = dof("g"), dof("uhat")
    prob = solvers.LinearSourceControl(V, Nt, dt, velocity, eps=eps)
    try:
        t0 = time.perf_counter()
        u, p, c, hist = solvers.pgd_source_control(prob, dof("u")[:n], uhat, np.zeros((Nt + 1) * n), beta,
                                                   c_lower, c_upper, g=g, increment=args.increment, tol=1e-4)
        el = time.perf_counter() - t0
    finally:
        prob.close()
    err = solvers.source_control_errors(V, u, c, p, lambda t: exact(t, X, Y), dx, dt, hist["iterations"])
    print(f"dx={dx}, dt={dt:g}, T={T}, beta={beta}: {hist['iterations']} iterations in {el:.2f} s, "
          f"J_acc {hist['cost'][-1]:.4e}, re-solved J {hist['cost_state'][-1]:.4e}")
    print(err["csv"])
