#!/usr/bin/env python3
"""Drift control with four actuators: the all-time solid-body problem (a Gaussian carried by the rotation, target = the
build's own forward solve at the drift strength c = 2) with a control that is constant in space on a 2 x 2 layout of
blocks and does not act on a margin of nodes along the boundary, ``control_space=ControlZones.blocks(...)``.  Every time
level has four amplitudes; the direction is the steepest-descent direction among such controls, an m x m solve per level
in place of the free control's mass solve.  Prints the amplitude table.

  python examples/zone_control_pdeco.py [--iters 5]        # 41 x 41 nodes, 50 steps, margin 4
  python examples/zone_control_pdeco.py --reduced          # 21 x 21 nodes, 6 steps, margin 2: a few seconds"""
import argparse
import time

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--reduced", action="store_true")
args = ap.parse_args()

nc, Nt, margin = (20, 6, 2) if args.reduced else (40, 50, 4)
dt = 1e-3 * 80 / nc
V = hp.SquareMeshP1(-1.0, 1.0, nc)
n = V.nodes
tl = (Nt + 1) * n
order = hp.ORDER_VERTEX
X, Y = V.coordinates()
u0 = np.exp(-15 * ((X + 0.2) ** 2 + (Y - 0.1) ** 2))
zones = solvers.ControlZones.blocks(V, 2, 2, margin=margin, order=order)
prob = solvers.SolidBodyDrift(V, Nt, dt, om=np.pi / 40, order=order)
try:
    target = np.concatenate([u0, np.zeros(tl - n)])
    prob.solve_state(np.full(tl, 2.0), target)
    c0 = np.ones(tl)
    t0 = time.perf_counter()
    u, p, c, hist = solvers.pgd_solidbody_alltime(prob, u0, target, c0, 0.01, 0.0, 5.0, args.iters, s0=8.0, max_armijo=6,
                                                  control_space=zones)
    el = time.perf_counter() - t0
finally:
    prob.close()
print(f"solid body, {zones.m} zones of {list(zones.sizes)} nodes, {int((~zones.active).sum())} nodes without control: "
      f"{len(hist['cost'])} PGD iterations in {el:.2f} s")
for k, J in enumerate(hist["cost"]):
    print(f"  it {k + 1:2d}  J = {J:.8e}   Armijo trials {hist['armijo_k'][k]}")
a = zones.compact(c, n)
print(f"constant on the zones: {zones.contains(c, n)}, untouched elsewhere: "
      f"{bool(np.all(c.reshape(-1, n)[:, ~zones.active] == 1.0))}")
print("amplitudes (level: zone 0 .. 3; the target was made with c = 2)")
for l in sorted({0, Nt // 2, Nt} | set(range(0, Nt + 1, max(1, Nt // 6)))):
    print(f"  level {l:3d}: " + "  ".join(f"{v:9.6f}" for v in a[l]))
