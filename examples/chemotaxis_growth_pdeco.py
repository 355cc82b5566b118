#!/usr/bin/env python3
"""Chemotaxis with cell growth (Mimura-Tsujikawa) on the MI355X backend: a forward pattern run and a few projected
gradient iterations with the per-step control.

    du/dt + div(-Dm grad u + chi u exp(-eta u) grad v) = r(u),   r(u) = u (r0 + r1 u + r2 u^2)

`--growth 0 1 -1` (default) is m^2 (1 - m) of mimura_data_helpers.py:70, `--growth 4 -1 0` the m (4 - m) of the header of
chemotaxis_mimura_FCT_PGD_alltime.py; the reaction term is explicit in time (IMEX), as the reference runs it.  Targets:
the build's own forward solve at the true control, as the reference workflow does.

usage: python examples/chemotaxis_growth_pdeco.py [--nodes 41] [--pattern-steps 400] [--steps 200] [--iters 2]
                                                  [--growth R0 R1 R2]"""
import argparse
import time

import numpy as np

from _common import hp

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=41, help="nodes per side of the unit square")
ap.add_argument("--pattern-steps", type=int, default=400)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--growth", type=float, nargs=3, default=[0.0, 1.0, -1.0], metavar=("R0", "R1", "R2"))
args = ap.parse_args()

dt, growth = 5e-4, tuple(args.growth)
V = hp.SquareMeshP1(0.0, 1.0, args.nodes - 1)
n = V.nodes
u0, v0 = hp.chtxs_sys_IC(0, 1, 1.0 / (args.nodes - 1), n, V.vertex_to_dof)

# forward pattern run with the constant control c = 10 (generation mode takes one control level), with and without growth
z = lambda x0, Nt: np.concatenate([x0, np.zeros(Nt * n)])
Np = args.pattern_steps
c_const = np.full((Np + 1) * n, 10.0)
t0 = time.perf_counter()
ug, vg = hp.solve_chtxs_system(c_const, z(u0, Np), z(v0, Np), V, n, Np, dt, None, growth=growth)
el = time.perf_counter() - t0
uf, _ = hp.solve_chtxs_system(c_const, z(u0, Np), z(v0, Np), V, n, Np, dt, None)
end = lambda a: a[Np * n:]
print(f"pattern run: {Np} steps of dt = {dt} with growth {growth} in {el:.2f} s")
print(f"  cells at T = {Np * dt:g}: min {end(ug).min():.4f}  mean {end(ug).mean():.4f}  max {end(ug).max():.4f}"
      f"   (growth-free: min {end(uf).min():.4f}  mean {end(uf).mean():.4f}  max {end(uf).max():.4f})")

# projected gradient descent towards the trajectory of the true control, the state stepped with the control of its level
Nt = args.steps
ut, vt = hp.solve_chtxs_system(np.full((Nt + 1) * n, 10.0), z(u0, Nt), z(v0, Nt), V, n, Nt, dt, None, growth=growth,
                               control_per_step=True)
t0 = time.perf_counter()
res = hp.projected_gradient_descent("chtxs", V, (u0, v0), (ut.copy(), vt.copy()), Nt, dt, speculative=True,
                                    control_per_step=True, growth=growth, max_iter_GD=args.iters, tol=0.0)
el = time.perf_counter() - t0
print(f"chtxs with growth (alltime): {res['it']} PGD iterations in {el:.2f} s, restored = {res['restored']}")
for k, J in enumerate(res["cost"]):
    trials = res["armijo_its"][k - 1] if k else "-"
    print(f"  it {k:2d}  J = {J:.8e}   Armijo trials {trials}")
