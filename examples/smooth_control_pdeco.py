#!/usr/bin/env python3
"""Smooth controls: the drift-control problem (rotation + drift control b = (1,1), c in [0,5], final-time tracking) from a
start control that oscillates in space and time, with and without the H1 regularisation

    R(c) = beta_x/2 int int |grad c|^2 + beta_t/2 int int (dc/dt)^2

on top of beta/2 ||c||^2_Q, by projected gradient descent.  Both runs record the roughness R_x = int int |grad c|^2 and
R_t = int int (dc/dt)^2 of every accepted iterate (``Smoothness(0, 0)`` changes no iterate and only records them): without
the term the gradient steps leave the start's oscillation in time nearly as it is and add roughness in space; with it
both go down.

usage: python examples/smooth_control_pdeco.py [--reduced] [--iters 4] [--trials 8] [--beta-x BX] [--beta-t BT]
(--reduced: 21 x 21 nodes and 20 steps of 2e-3 in place of 81 x 81 and 100 of 1e-3; the default coefficients follow the
mesh, beta_x ~ h^2 and beta_t ~ dt^2: 2e-4, 4e-7 reduced and 5e-5, 1e-7 at full size)"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--reduced", action="store_true")
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--trials", type=int, default=8)
ap.add_argument("--beta-x", type=float, default=None)
ap.add_argument("--beta-t", type=float, default=None)
args = ap.parse_args()

nc, Nt, dt = (20, 20, 2e-3) if args.reduced else (80, 100, 1e-3)
beta_x = args.beta_x if args.beta_x is not None else (2e-4 if args.reduced else 5e-5)
beta_t = args.beta_t if args.beta_t is not None else (4e-7 if args.reduced else 1e-7)
beta, c_lower, c_upper = 0.05, 0.0, 5.0
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
n = mesh.nodes
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, eps=0.0, drift=(1.0, 1.0), order=hp.ORDER_VERTEX)
x, y = mesh.coordinates()                           # vertex order, the device's
u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
t = np.arange(Nt + 1)[:, None] * dt
ref = np.zeros((Nt + 1) * n)
ref[:n] = u0
prob.solve_state((1.5 + np.sin(2 * x)[None] * np.cos(y + 5 * t)).ravel(), ref)
uhat_T = ref[Nt * n:]
c0 = (0.5 + 0.3 * np.sin(6 * x)[None] * np.cos(5 * y)[None] * np.cos(0.8 / dt * t)).ravel()     # rough in space and time

t0 = time.perf_counter()
for name, sm in (("plain ", solvers.Smoothness(0.0, 0.0)), ("smooth", solvers.Smoothness(beta_x, beta_t))):
    u, p, c, hist = solvers.pgd_solidbody(prob, u0, uhat_T, c0, beta, c_lower, c_upper, args.iters, max_armijo=args.trials,
                                          optim="finaltime", smoothness=sm)
    fmt = lambda v: " ".join(f"{a:.6e}" for a in v)
    print(f"{name} beta_x = {sm.beta_x:g} beta_t = {sm.beta_t:g}  J + R = {hist['cost'][-1]:.8e}  Armijo trials {hist['armijo_k']}")
    print(f"{name} roughness_x: {fmt(hist['roughness_x'])}")
    print(f"{name} roughness_t: {fmt(hist['roughness_t'])}")
print(f"{n} nodes, {Nt} steps: two runs of {args.iters} PGD iterations in {time.perf_counter() - t0:.2f} s")
prob.close()
