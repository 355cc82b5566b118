#!/usr/bin/env python3
"""Snapshot tracking: config C2's set-up (advection_solidbody_FCT_PDECO_finaltime.py: [-1,1]^2, 81 x 81 P1 nodes,
dt = 1e-3, rotation + drift control b = (1,1), c in [0,5], beta = 1, slotted disc) run to T = 0.5 with the two shipped
snapshots data/solidbody_t0.25_u.csv and data/solidbody_t0.5_u.csv (tests/golden/ref_data/) as observations of one
trajectory, J = 1/2 sum_{t in {0.25, 0.5}} ||u(t) - uhat(t)||^2_M + beta/2 ||c||^2_Q, by projected gradient descent.

usage: python examples/solidbody_snapshots_pdeco.py [--iters 5] [--steps 500] [--trials 10]
(--steps N: N time steps, the snapshots at levels N/2 and N -- a reduced run for a quick look)"""
import argparse
import os
import time

import numpy as np

from _common import ROOT, hp, solvers, slotted_disc, to_dof

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--trials", type=int, default=10)
args = ap.parse_args()

a1, a2, dx, dt = -1.0, 1.0, 0.1 / 2 / 2, 0.001
beta, c_lower, c_upper = 1.0, 0.0, 5.0
mesh = hp.SquareMeshP1(a1, a2, round((a2 - a1) / dx))
n, Nt = mesh.nodes, args.steps
data = os.path.join(ROOT, "tests", "golden", "ref_data")
obs = solvers.Observations(Nt, [Nt // 2, Nt])
uhat = np.full((Nt + 1) * n, np.nan)                # only the observed levels are read
for lv, name in zip(obs.levels, ("solidbody_t0.25_u.csv", "solidbody_t0.5_u.csv")):
    uhat[lv * n:(lv + 1) * n] = hp.import_data_final(os.path.join(data, name), n, mesh.vertex_to_dof)[1]
u0 = to_dof(mesh, slotted_disc(a1, a2, dx))
c0 = np.zeros((Nt + 1) * n)

prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, eps=0.0, drift=(1.0, 1.0), order=hp.ORDER_VERTEX)
dev = lambda x: hp.reorder_vector_from_dof(x, x.size // n, n, mesh.vertex_to_dof)          # device works in vertex order
t0 = time.perf_counter()
u, p, c, hist = solvers.pgd_solidbody_snapshots(prob, dev(u0), dev(uhat), obs, dev(c0), beta, c_lower, c_upper, args.iters,
                                                max_armijo=args.trials)
el = time.perf_counter() - t0
for k, (J, a, s) in enumerate(zip(hist["cost"], hist["armijo_k"], hist["step"])):
    print(f"it {k + 1:3d}  J = {J:.8e}  Armijo trials {a:2d}  step {s:g}")
print(f"snapshots at levels {[int(lv) for lv in obs.levels]} of {Nt}: {len(hist['cost'])} PGD iterations in {el:.2f} s")
prob.close()
