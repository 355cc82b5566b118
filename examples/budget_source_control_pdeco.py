#!/usr/bin/env python3
"""The manufactured source-control problem of examples/sparse_source_control_pdeco.py (unit square, dt = dx^2, eps = 1e-3,
beta = 1e-3, the exact g, uhat and u0, box [-0.1, 0.5]) with a control budget instead of an L1 penalty: minimise J(u, c)
subject to ||c||_{1,h} <= B by projected gradient descent onto the budget set (solvers.prox_source_control with alpha = 0
and budget=B, an extension with no counterpart in the reference).  B is a fraction of the norm the unconstrained run
reaches in the same number of iterations.  The multiplier of the constraint is the L1 weight that meets the budget, so the
control comes out sparse without tuning alpha: the run prints, per iteration, the cost, the L1 norm, the multiplier and
the share of nonzero control values.

usage: python examples/budget_source_control_pdeco.py [--iters 10] [--dx 0.1] [--fraction 0.3] [--s0 64]"""
import argparse

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--dx", type=float, default=0.1)
ap.add_argument("--fraction", type=float, default=0.3)
ap.add_argument("--s0", type=float, default=64.0)
args = ap.parse_args()

T, eps, beta, c_lower, c_upper, e1, e2 = 1.0, 1e-3, 1e-3, -0.1, 0.5, 0.2, 0.3


def velocity(x, y):
    """advection_FCT_PDECO_alltime_exact.py:132-135"""
    return 2 * (y - 0.5) * x * (1 - x), -2 * (x - 0.5) * y * (1 - y)


def exact(t, X, Y):
    """uex, gex, uhatex of advection_FCT_PDECO_alltime_exact.py:77-128 (k1 = k2 = 1, the script's bounds [0, 0.5])"""
    pi = np.pi
    sx, sy, cx, cy = np.sin(pi * X), np.sin(pi * Y), np.cos(pi * X), np.cos(pi * Y)
    u = np.exp(e1 * t) * (sx * sy) ** 2
    amp = np.exp(e2 * T) - np.exp(e2 * t)
    c = np.clip(amp * (sx * sy) ** 2 / beta, 0.0, 0.5)
    wx, wy = velocity(X, Y)
    lap_u = 2 * pi ** 2 * np.exp(e1 * t) * (np.cos(2 * pi * X) * sy ** 2 + sx ** 2 * np.cos(2 * pi * Y))
    g = e1 * u - eps * lap_u + wx * 2 * pi * np.exp(e1 * t) * sx * cx * sy ** 2 \
        + wy * 2 * pi * np.exp(e1 * t) * sx ** 2 * sy * cy - c
    lap_p = 2 * pi ** 2 * amp * (np.cos(2 * pi * X) * sy ** 2 + sx ** 2 * np.cos(2 * pi * Y))
    uhat = e2 * np.exp(e2 * t) * (sx * sy) ** 2 - eps * lap_p - wx * 2 * pi * amp * sx * cx * sy ** 2 \
        - wy * 2 * pi * amp * sx ** 2 * sy * cy + u
    return dict(u=u.ravel(), g=g.ravel(), uhat=uhat.ravel())


dx = args.dx
nc = round(1.0 / dx)
V = hp.SquareMeshP1(0.0, 1.0, nc)
n, dt = V.nodes, dx ** 2
Nt = round(T / dt)
grid = np.arange(0.0, 1.0 + dx, dx)[:nc + 1]
X, Y = np.meshgrid(grid, grid)
fields = [exact(i * dt, X, Y) for i in range(Nt + 1)]
dof = lambda key: hp.reorder_vector_to_dof_time(np.concatenate([f[key] for f in fields]), Nt + 1, n, V.vertex_to_dof)
g, uhat, u0 = dof("g"), dof("uhat"), dof("u")[:n]
prob = solvers.LinearSourceControl(V, Nt, dt, velocity, eps=eps)
try:
    run = lambda **kw: solvers.prox_source_control(prob, u0, uhat, np.zeros((Nt + 1) * n), beta, 0.0, c_lower, c_upper, g=g,
                                                   s0=args.s0, max_iters=args.iters, **kw)
    free = run()[3]
    if not free["l1"]:
        raise SystemExit("the unconstrained run accepted no step")
    B = args.fraction * free["l1"][-1]
    print(f"unconstrained: ||c||_(1,h) = {free['l1'][-1]:.8e}, J = {free['cost'][-1]:.8e}, nonzero "
          f"{free['nonzero_fraction'][-1]:.4f} after {free['iterations']} iterations")
    u, p, c, h = run(budget=B)
    print(f"projected gradient with the budget ||c||_(1,h) <= {B:.8e} ({args.fraction:g} of that): dx = {dx}, {Nt} steps, "
          f"box [{c_lower}, {c_upper}], s0 = {args.s0:g}, J(c0) = {h['cost0']:.8e}")
    print("  it  sweeps  J                 l1                multiplier        nonzero  rounds  trials")
    for k in range(h["iterations"]):
        print(f"{k + 1:4d}  {h['sweeps'][k]:6d}  {h['cost'][k]:.8e}  {h['l1'][k]:.8e}  {h['multiplier'][k]:.8e}  "
              f"{h['nonzero_fraction'][k]:7.4f}  {h['projection_rounds'][k]:6d}  {h['armijo_k'][k]:6d}")
    if h["stalled"]:
        print("no trial passed the Armijo test: stopped")
    print(f"final control: {np.mean(c == c_lower):.3f} at the lower bound, {np.mean(c == c_upper):.3f} at the upper bound, "
          f"{np.mean(c == 0):.3f} exactly zero; budget used {h['budget_used'][-1] if h['budget_used'] else 0.0:.6f}")
finally:
    prob.close()
