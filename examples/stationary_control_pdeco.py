#!/usr/bin/env python3
"""Parameter identification for the advective Schnakenberg system: the refactored driver's problem
(Schnak_FCT_PDECO_refactored.py: UnitSquare, final-time misfit, control box [0, 10]) with its default forward sweep, which
freezes the control at time level 1 (helpers.py:577-578), paired with a control that does not depend on time,
``control_time=ControlIntervals.stationary``.  The state depends on one spatial field, so that is the problem the sweep
poses; the direction is the time average of the pointwise expression -(beta c - gamma/r p), the gradient with respect to
the one field.  Target: the build's own forward solve at the true parameter a = 0.1.

  python examples/stationary_control_pdeco.py [--iters 5]       # 41 x 41 nodes, dt = 5e-4, T = 0.1
  python examples/stationary_control_pdeco.py --reduced         # 13 x 13 nodes, 8 steps of 1e-3: a few seconds"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--reduced", action="store_true")
args = ap.parse_args()

dx, dt, Nt = (1 / 12, 1e-3, 8) if args.reduced else (0.025, 5e-4, 200)
V = hp.SquareMeshP1(0.0, 1.0, round(1 / dx))
n = V.nodes
tl = (Nt + 1) * n
z = lambda x0: np.concatenate([x0, np.zeros(Nt * n)])
ic = hp.schnak_sys_IC(0, 1, dx, n, V.vertex_to_dof)
full = hp.solve_schnak_system(np.full(tl, 0.1), z(ic[0]), z(ic[1]), V, n, Nt, dt, None)
targets = tuple(np.array(f[Nt * n:]) for f in full)
ct = solvers.ControlIntervals.stationary(Nt)
t0 = time.perf_counter()
res = hp.projected_gradient_descent("schnak", V, ic, targets, Nt, dt, control_time=ct, max_iter_GD=args.iters, tol=0.0,
                                    max_iter_armijo=14)
el = time.perf_counter() - t0
print(f"schnak, stationary control, frozen sweep: {res['it']} PGD iterations in {el:.2f} s, restored = {res['restored']}")
for k, J in enumerate(res["cost"]):
    trials = res["armijo_its"][k - 1] if k else "-"
    print(f"  it {k:2d}  J = {J:.8e}   Armijo trials {trials}")
a = ct.compact(res["c"], n)
print(f"control: {a.shape[0]} field of {a.shape[1]} values, constant in time: {ct.contains(res['c'], n)}, "
      f"range [{a.min():.6f}, {a.max():.6f}] (true parameter 0.1)")
