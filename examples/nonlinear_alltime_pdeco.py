#!/usr/bin/env python3
"""The all-time PDECO of the nonlinear advection-reaction equation, nonlinear_FCT_PDECO_alltime.py, on the MI355X backend:
UnitSquare with dx = 0.025 (41 x 41 P1 nodes), dt = 1e-3, T = 0.5 (500 forward + 500 adjoint steps per solve), beta = 0.1,
c in [-1, 1], tol 1e-4 (:40-55).  The state step to level n+1 reads control level n+1 (:189-192, ``control_per_step``),
the adjoint has p(T) = 0 and the misfit load M (uhat_n - u_n) in every step (:198-216, with HEAD's M_u2(u_n)).

Target: the build's own per-step forward solve at c = sin(2 pi x) sin(2 pi y) on every level, the control of the target
generator nonlinear_generate_pattern_FCT.py:48-50, 83-85, 92-93 (whose solve is commented out at HEAD).

usage: python examples/nonlinear_alltime_pdeco.py [--iters 3] [--sequential]"""
import argparse
import time

import numpy as np

from _common import hp

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--sequential", action="store_true", help="one Armijo trial at a time instead of the speculative batch")
args = ap.parse_args()

a1, a2, dx, dt, T = 0.0, 1.0, 0.025, 1e-3, 0.5
V = hp.SquareMeshP1(a1, a2, round((a2 - a1) / dx))
n, Nt = V.nodes, round(T / dt)
tl = (Nt + 1) * n
u0 = hp.nonlinear_equation_IC(a1, a2, dx, n, V.vertex_to_dof)
X, Y = np.meshgrid(np.arange(a1, a2 + dx, dx), np.arange(a1, a2 + dx, dx))
source = hp.reorder_vector_to_dof((np.sin(2 * np.pi * X) * np.sin(2 * np.pi * Y)).reshape(n), 1, n, V.vertex_to_dof)
uhat = np.zeros(tl)
uhat[:n] = u0
hp.solve_nonlinear_equation(np.tile(source, Nt + 1), uhat, None, V, n, Nt, dt, None, control_per_step=True)

t0 = time.perf_counter()
res = hp.projected_gradient_descent("nonlinear", V, (u0,), (uhat,), Nt, dt, speculative=not args.sequential,
                                    control_per_step=True, optim="alltime", max_iter_GD=args.iters)
el = time.perf_counter() - t0
print(f"nonlinear (alltime, per-step control): {res['it']} PGD iterations in {el:.2f} s, restored = {res['restored']}")
for k, J in enumerate(res["cost"]):
    trials = res["armijo_its"][k - 1] if k else "-"
    print(f"  it {k:2d}  J = {J:.8e}   Armijo trials {trials}")
print(f"cost {res['cost'][0]:.6e} -> {res['cost'][-1]:.6e}")
