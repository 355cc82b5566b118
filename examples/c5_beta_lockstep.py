#!/usr/bin/env python3
"""Config C5 as ONE lockstep loop: the regularisation sweep of advection_solidbody_FCT_PDECO_alltime.py:43-74 (the
reference ran one edited script copy per beta) with all eight beta carried by solvers.pgd_solidbody_lockstep, so that
every launch of an iteration advances all problems, or all problems x Armijo trials.  Set-up and table as
c5_beta_sweep.py, which runs one beta after another.  Under torch.distributed.run each rank runs the share of beta that
sweep.sweep_batched deals it as one lockstep loop; the only exchange is an all-gather of the final costs.

  python examples/c5_beta_lockstep.py                                 # all 8 values in one loop on one GPU
  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 examples/c5_beta_lockstep.py"""
import argparse
import os

import numpy as np

from _common import hp, solvers, sweep, gaussian

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--steps", type=int, default=100, help="time steps of dt = 1e-3 (config C5: 100, T = 0.1)")
args = ap.parse_args()
world = int(os.environ.get("WORLD_SIZE", "1"))
local_rank = int(os.environ.get("LOCAL_RANK", "0"))
dist = None
if world > 1:
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local_rank)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

a1, a2, dx, dt = -1.0, 1.0, 0.025, 0.001
mesh = hp.SquareMeshP1(a1, a2, round((a2 - a1) / dx))
n, Nt = mesh.nodes, args.steps
tl = (Nt + 1) * n
prob = solvers.SolidBodyDrift(mesh, Nt, dt, eps=0.0, drift=(1.0, 1.0), rot_scale=0.0, device_id=local_rank,
                              order=hp.ORDER_VERTEX)
u0 = gaussian(a1, a2, dx)                       # vertex order = device order
uhat = np.zeros(tl)
uhat[:n] = u0
uhat = prob.solve_state(2.0 * np.ones(tl), uhat)          # target trajectory at the true control c = 2
betas = [10.0 ** (-k / 2) for k in range(8)]


def run(mine):
    res = solvers.pgd_solidbody_lockstep(prob, u0, uhat, np.ones(tl), mine, 0.0, 5.0, args.iters, optim="alltime")
    return [hist["cost"][-1] for _, _, _, hist in res]


costs = sweep.sweep_batched(betas, run, dist)
if int(os.environ.get("RANK", "0")) == 0:
    for b, J in zip(betas, costs):
        print(f"beta = {b:9.3e}   J after {args.iters} PGD iterations = {J:.8e}")
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
prob.close()
