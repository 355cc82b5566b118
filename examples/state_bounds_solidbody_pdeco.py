#!/usr/bin/env python3
"""State bounds: the drift-control problem (rotation + drift control b = (1,1), c in [0,5], final-time tracking) with an
upper bound u <= u_max on the state as a Moreau-Yosida penalty,

    J_gamma = 1/2 ||u(T) - uhat_T||^2_M + beta/2 ||c||^2_Q + gamma/2 dt sum_n sum_i ml_i max(u_{n,i} - u_max, 0)^2,

by projected gradient descent with a continuation over three values of gamma, each stage warm-started with the control
of the one before.  The target is the final state under a reference control.  The initial Gaussian (height 1) itself
exceeds u_max, so the largest violation stays at the first levels' whatever the control does; the measure that shows
the continuation work is the weighted violation P/gamma.

usage: python examples/state_bounds_solidbody_pdeco.py [--reduced] [--iters 3] [--trials 6] [--umax 0.3]
(--reduced: 21 x 21 nodes and 20 steps in place of 81 x 81 and 100)"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--reduced", action="store_true")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--trials", type=int, default=6)
ap.add_argument("--umax", type=float, default=0.3)
ap.add_argument("--gammas", type=float, nargs=3, default=[50.0, 500.0, 5000.0])
args = ap.parse_args()

nc, Nt, dt = (20, 20, 2e-3) if args.reduced else (80, 100, 1e-3)
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

bounds = solvers.StateBounds(Nt, upper=args.umax, gamma=args.gammas[0])
c = np.full((Nt + 1) * n, 0.5)
t0 = time.perf_counter()
for gamma in args.gammas:
    b = bounds.with_gamma(gamma)
    u, p, c, hist = solvers.pgd_solidbody(prob, u0, uhat_T, c, beta, c_lower, c_upper, args.iters, max_armijo=args.trials,
                                          optim="finaltime", state_bounds=b)
    P = hist["penalty"][-1]
    print(f"gamma {gamma:g}  J_gamma = {hist['cost'][-1]:.8e}  penalty = {P:.8e}  penalty/gamma = {P / gamma:.8e}  "
          f"max violation = {hist['max_violation'][-1]:.4f}  violated = {100 * hist['violated_fraction'][-1]:.2f} %  "
          f"Armijo trials {hist['armijo_k']}")
print(f"u <= {args.umax:g} on {n} nodes, {Nt} steps: {len(args.gammas)} continuation stages of {args.iters} PGD iterations "
      f"in {time.perf_counter() - t0:.2f} s")
prob.close()
