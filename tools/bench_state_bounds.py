#!/usr/bin/env python3
"""Adjoint sweep and batched trial costing of the drift-control problem with and without state bounds, on one context:
graph replay, median of --reps runs after warm-up, one process.  A step with bounds has the launches of the snapshot
sweep, with k_bound_load in the place of k_obs_load; the costing adds one fused pass (k_bound_cost_part / _finish) to
the cost of a batch of trials.  The snapshot sweep is timed twice (before and after): the ratio of those two medians is
the spread of a repeated run on the box, the yardstick for the other ratio.  obs_ms stands in for the snapshot sweep of
the commit before the bounds (what tools/bench_snapshots.py prints as obs_3_ms): that sweep's kernels, k_obs_load
among them, have the same machine code in this build (profiles/kernel_fingerprints.txt), and timing both sweeps in
one process on one box removes the box-to-box difference that a number carried over from an older run would bring.

  obs_ms / obs2_ms     femfct_solidbody_adjoint_obs, three snapshots (levels Nt/4, Nt/2, Nt), first and second timing
  bounds_ms            femfct_solidbody_adjoint_bounds, the same snapshots and two-sided bounds at every level
  cost_ms / costb_ms   SolidBodyDrift.cost of the batch without and with the bounds' statistics

usage: python tools/bench_state_bounds.py [--reps 30] > profiles/state_bounds.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hp = importlib.import_module("fem-fct-pdeco_amd")
solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()                     # a sweep returns after it has read its solver log, a cost after its read-back: synchronised
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


print(f"# build {hp._lib.lib.femfct_build_id().decode()}: adjoint sweep and trial costing, 40 steps, median of {args.reps} "
      f"runs after {args.warmup}; ms per run")
print("# obs_ms / obs2_ms: the snapshot sweep without bounds in this build and process (the kernels of the commit before, "
      "unchanged code), timed before and after bounds_ms")
print("# nodes batch  obs_ms  obs2_ms  bounds_ms  spread  bounds/obs  cost_ms  costb_ms  violated")
Nt = 40
for nc, batches in ((20, (1, 10)), (80, (1, 10)), (256, (1,))):
    V = hp.SquareMeshP1(-1.0, 1.0, nc)
    n, dt = V.nodes, 1e-3 * 80 / nc
    tl = (Nt + 1) * n
    rng = np.random.default_rng(nc)
    x, y = V.coordinates()
    prob = solvers.SolidBodyDrift(V, Nt, dt, batch=max(batches), order=hp.ORDER_VERTEX)
    obs = solvers.Observations(Nt, [Nt // 4, Nt // 2, Nt])
    bounds = solvers.StateBounds(Nt, lower=0.001, upper=0.3, gamma=200.0)
    try:
        for B in batches:
            ctx = prob.ctx
            c = ctx.array(2.0 * rng.random(B * tl))
            u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
            u = ctx.array(np.tile(np.concatenate([u0, np.zeros(tl - n)]), B))
            prob.forward(c, u, batch=B)
            uh = ctx.array(0.9 * u.download() + 0.01)
            p = ctx.zeros(B * tl)
            t_o = median_ms(lambda: prob.adjoint(c, u, uh, p, "snapshots", batch=B, obs=obs))
            t_b = median_ms(lambda: prob.adjoint(c, u, uh, p, "snapshots", batch=B, obs=obs, state_bounds=bounds))
            t_o2 = median_ms(lambda: prob.adjoint(c, u, uh, p, "snapshots", batch=B, obs=obs))
            t_c = median_ms(lambda: prob.cost(u, uh, c, 0.1, "snapshots", batch=B, obs=obs))
            t_cb = median_ms(lambda: prob.cost(u, uh, c, 0.1, "snapshots", batch=B, obs=obs, state_bounds=bounds))
            frac = prob.bound_stats(u, bounds, batch=B)[2][0]
            print(f"{nc + 1}^2 {B:3d}  {t_o:9.3f}  {t_o2:9.3f}  {t_b:9.3f}  {t_o2 / t_o:.3f}  {t_b / min(t_o, t_o2):.3f}  "
                  f"{t_c:8.3f}  {t_cb:8.3f}  {100 * frac:.1f} %")
            for a in (c, u, uh, p):
                a.free()
    finally:
        prob.close()
