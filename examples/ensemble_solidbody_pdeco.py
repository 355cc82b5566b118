#!/usr/bin/env python3
"""One drift control for three scenarios (solvers.ensemble_solidbody, an extension with no counterpart in the reference):
[-1,1]^2, 41 x 41 P1 nodes, 40 steps of 5e-3, rotation + drift control, c in [0, 5], beta = 1e-3.  Three initial blobs
exp(-15 |x - x_s|^2) with the probabilities (0.5, 0.3, 0.2); the target of scenario s is its own state at T under the
constant control 1.5, 2.0, 2.5 (final-time tracking).  Prints the ensemble cost per iteration, the per-scenario costs
at the robust control, and what the optimum of scenario 0 alone (solvers.lbfgs_solidbody) costs the other scenarios.

usage: python examples/ensemble_solidbody_pdeco.py [--iters 8] [--memory 3]"""
import argparse

import numpy as np

from _common import hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--memory", type=int, default=3)
args = ap.parse_args()

nc, Nt, dt = 40, 40, 5e-3
beta, c_lower, c_upper, s0 = 1e-3, 0.0, 5.0, 64.0
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
n = mesh.nodes
tl = (Nt + 1) * n
x, y = mesh.coordinates()                      # the device works in vertex order here
centres, weights = [(-0.2, 0.1), (0.1, -0.2), (0.0, 0.3)], [0.5, 0.3, 0.2]
u0 = np.stack([np.exp(-15 * ((x - a) ** 2 + (y - b) ** 2)) for a, b in centres])

prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, eps=0.0, drift=(1.0, 1.0), order=hp.ORDER_VERTEX)
uhat = []
for s, cv in enumerate((1.5, 2.0, 2.5)):
    traj = np.zeros(tl)
    traj[:n] = u0[s]
    prob.solve_state(np.full(tl, cv), traj)
    uhat.append(traj[Nt * n:].copy())
uhat = np.stack(uhat)
c0 = np.ones(tl)

ens = solvers.Ensemble(u0, uhat, weights)
u, p, c, h = solvers.ensemble_solidbody(prob, ens, c0, beta, c_lower, c_upper, args.iters, memory=args.memory, s0=s0)
print(f"ensemble cost: J(c0) = {h['cost0']:.8e}, scenario costs at c0 = " + "  ".join(f"{t:.4e}" for t in h["scenario_costs0"]))
print("  it  sweeps  J                 trials  used   worst T_s     control cost")
for k in range(len(h["cost"])):
    print(f"{k + 1:4d}  {h['sweeps'][k]:6d}  {h['cost'][k]:.8e}  {h['armijo_k'][k]:6d}  {h['used'][k]:>4s}   {h['worst'][k]:.4e}    "
          f"{h['control_cost'][k]:.4e}")
robust = h["scenario_costs"][-1] if h["scenario_costs"] else h["scenario_costs0"]

# scenario 0's own optimum, and what it costs the others: one cost pass of the three scenarios under that control
_, _, c_own, h_own = solvers.lbfgs_solidbody(prob, u0[0], uhat[0], c0, beta, c_lower, c_upper, args.iters,
                                             memory=max(args.memory, 1), s0=s0, optim="finaltime")
obs = solvers.Observations.finaltime(Nt)
_, cost_w, _ = prob.obs_device(obs)
ctx = prob.ctx
cd, ud, hd = ctx.array(c_own), ctx.zeros(3 * tl), ctx.zeros(3 * tl)
ud.upload(np.concatenate([np.concatenate([u0[s], np.zeros(tl - n)]) for s in range(3)]))
hd.upload(np.concatenate([np.concatenate([np.zeros(tl - n), uhat[s]]) for s in range(3)]))
prob.forward(cd, ud, batch=3, c_shared=True)
own, J_own, _ = ctx.ensemble_costs(ud, hd, cost_w, cd, ens.weights, beta, Nt, dt)
print("per-scenario tracking costs T_s          scenario 0      scenario 1      scenario 2      ensemble J")
print("  robust control                         " + "  ".join(f"{t:.6e}" for t in robust) + f"    {(h['cost'] or [h['cost0']])[-1]:.6e}")
print("  scenario 0's own optimum               " + "  ".join(f"{t:.6e}" for t in own) + f"    {J_own:.6e}")
prob.close()
