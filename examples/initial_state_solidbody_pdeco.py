#!/usr/bin/env python3
"""Initial-state recovery (data assimilation): which state at t = 0 produced the two shipped snapshots
data/solidbody_t0.25_u.csv and data/solidbody_t0.5_u.csv (tests/golden/ref_data/) of one trajectory?  Config C2's set-up
(advection_solidbody_FCT_PDECO_finaltime.py: [-1,1]^2, 81 x 81 P1 nodes, dt = 1e-3, rotation + drift b = (1,1)) run to
T = 0.5 under a fixed control c (--control, constant), the snapshots as observations,

    J(v) = 1/2 sum_{t in {0.25, 0.5}} ||u(t; v) - uhat(t)||^2_M + beta0/2 ||v - v_b||^2_M,    v in [0, 1],

by projected L-BFGS descent on v = u(0) (solvers.initial_state_solidbody), from the first snapshot as the first guess and
the background.

usage: python examples/initial_state_solidbody_pdeco.py [--iters 5] [--steps 500] [--trials 10] [--memory 5]
(--steps N: N time steps, the snapshots at levels N/2 and N -- a reduced run for a quick look)"""
import argparse
import os
import time

import numpy as np

from _common import ROOT, hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--trials", type=int, default=10)
ap.add_argument("--memory", type=int, default=5)
ap.add_argument("--control", type=float, default=0.0)
ap.add_argument("--beta0", type=float, default=1e-4)
args = ap.parse_args()

a1, a2, dx, dt = -1.0, 1.0, 0.1 / 2 / 2, 0.001
v_lower, v_upper = 0.0, 1.0
mesh = hp.SquareMeshP1(a1, a2, round((a2 - a1) / dx))
n, Nt = mesh.nodes, args.steps
data = os.path.join(ROOT, "tests", "golden", "ref_data")
obs = solvers.Observations(Nt, [Nt // 2, Nt])
uhat = np.full((Nt + 1) * n, np.nan)                # only the observed levels are read
for lv, name in zip(obs.levels, ("solidbody_t0.25_u.csv", "solidbody_t0.5_u.csv")):
    uhat[lv * n:(lv + 1) * n] = hp.import_data_final(os.path.join(data, name), n, mesh.vertex_to_dof)[1]
first = np.clip(uhat[obs.levels[0] * n:(obs.levels[0] + 1) * n], v_lower, v_upper)
c = np.full((Nt + 1) * n, args.control)

prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, eps=0.0, drift=(1.0, 1.0), order=hp.ORDER_VERTEX,
                              batch=args.trials)
dev = lambda x: hp.reorder_vector_from_dof(x, x.size // n, n, mesh.vertex_to_dof)          # device works in vertex order
t0 = time.perf_counter()
u, p, v, hist = solvers.initial_state_solidbody(prob, dev(c), dev(uhat), dev(first), args.beta0, v_lower, v_upper, args.iters,
                                                background=dev(first), memory=args.memory, max_armijo=args.trials,
                                                optim="snapshots", obs=obs)
el = time.perf_counter() - t0
print(f"   0  J = {hist['cost0']:.8e}  tracking {hist['tracking0']:.6e}  background {hist['background0']:.6e}")
for k, (J, T, B, a, used) in enumerate(zip(hist["cost"], hist["tracking"], hist["background"], hist["armijo_k"], hist["used"])):
    print(f"{k + 1:4d}  J = {J:.8e}  tracking {T:.6e}  background {B:.6e}  Armijo trials {a:2d}  direction {used}")
print(f"state at t = 0 from the snapshots at levels {[int(lv) for lv in obs.levels]} of {Nt}: {len(hist['cost'])} iterations in "
      f"{el:.2f} s, {int(np.sum(v == v_lower))} / {int(np.sum(v == v_upper))} of {n} values at the lower / upper bound"
      + (", stalled" if hist["stalled"] else ""))
prob.close()
