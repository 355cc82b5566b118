#!/usr/bin/env python3
"""Config C2's problem (advection_solidbody_FCT_PDECO_finaltime.py: [-1,1]^2, 81 x 81 P1 nodes, dt = 1e-3, T = 0.25,
rotation + drift control, c in [0,5], beta = 1, slotted disc, target tests/golden/solidbody_t0.25_u.npz) solved twice: by
the projected gradient loop of the reference script (solvers.pgd_solidbody_finaltime) and by projected L-BFGS
(solvers.lbfgs_solidbody, an extension with no counterpart in the reference).  Prints the cost against the number of
state and adjoint sweeps a sequential search needs (both loops evaluate their trials as one batch).

usage: python examples/lbfgs_solidbody_pdeco.py [--iters 15] [--memory 5]"""
import argparse
import os

import numpy as np

from _common import ROOT, hp, solvers, slotted_disc, to_dof

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--memory", type=int, default=5)
args = ap.parse_args()

a1, a2, dx, dt, T = -1.0, 1.0, 0.1 / 2 / 2, 0.001, 0.25
beta, c_lower, c_upper = 1.0, 0.0, 5.0
mesh = hp.SquareMeshP1(a1, a2, round((a2 - a1) / dx))
Nt = round(T / dt)
u0 = to_dof(mesh, slotted_disc(a1, a2, dx))
uhat_T = np.load(os.path.join(ROOT, "tests", "golden", "solidbody_t0.25_u.npz"))["u"]
c0 = np.zeros((Nt + 1) * mesh.nodes)

prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, eps=0.0, drift=(1.0, 1.0), order=hp.ORDER_VERTEX)
v2d = mesh.vertex_to_dof
dev = lambda x: hp.reorder_vector_from_dof(x, x.size // mesh.nodes, mesh.nodes, v2d)     # device works in vertex order
_, _, _, hg = solvers.pgd_solidbody_finaltime(prob, dev(u0), dev(uhat_T), dev(c0), beta, c_lower, c_upper, args.iters)
_, _, _, hq = solvers.lbfgs_solidbody(prob, dev(u0), dev(uhat_T), dev(c0), beta, c_lower, c_upper, args.iters,
                                      memory=args.memory, optim="finaltime")
# the reference loop: per iteration one adjoint sweep, the state of the unconditional first step, one state per trial
sweeps_g = np.cumsum([2 + k for k in hg["armijo_k"]])
print(f"projected gradient (pgd_solidbody_finaltime)      projected L-BFGS, memory {args.memory} (J(c0) = {hq['cost0']:.8e})")
print("  it  sweeps  J                 trials             it  sweeps  J                 trials  used  pairs  free")
for k in range(max(len(hg["cost"]), len(hq["cost"]))):
    left = f"{k + 1:4d}  {sweeps_g[k]:6d}  {hg['cost'][k]:.8e}  {hg['armijo_k'][k]:6d}" if k < len(hg["cost"]) else " " * 38
    right = (f"{k + 1:4d}  {hq['sweeps'][k]:6d}  {hq['cost'][k]:.8e}  {hq['armijo_k'][k]:6d}  {hq['used'][k]:>4s}  "
             f"{hq['pairs'][k]:5d}  {hq['free_fraction'][k]:.3f}") if k < len(hq["cost"]) else ""
    print(left + " " * 12 + right)
if hq["stalled"]:
    print("L-BFGS: no trial passed the Armijo test along -g either: stopped")
prob.close()
