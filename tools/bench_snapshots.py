#!/usr/bin/env python3
"""Adjoint sweep of the drift-control problem with observations against the all-time sweep on the same inputs, on one
context: graph replay, median of --reps sweeps after warm-up, one process.  A step has the same launches, with
k_obs_load in the place of k_mass_diff.  The all-time sweep is timed twice (before and after): the ratio of those two
medians is the spread of a repeated run on the box, the yardstick for the other ratios.

  alltime_ms / alltime2_ms   femfct_solidbody_adjoint(alltime = 1), first and second timing
  obs_all_ms                 femfct_solidbody_adjoint_obs with Observations.alltime (the same arithmetic)
  obs_3_ms                   three snapshots (levels Nt/4, Nt/2, Nt): the other levels' load writes zeros

usage: python tools/bench_snapshots.py [--reps 30] > profiles/r09_snapshots.txt"""
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
        fn()                     # a sweep returns after it has read its solver log: synchronised
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


print(f"# build {hp._lib.lib.femfct_build_id().decode()}: adjoint sweep, 40 steps, median of {args.reps} sweeps after "
      f"{args.warmup}; ms per sweep")
print("# nodes batch  alltime_ms  alltime2_ms  obs_all_ms  obs_3_ms  spread  obs_all/alltime  obs_3/alltime")
Nt = 40
for nc, batches in ((20, (1, 10)), (80, (1, 10)), (256, (1,))):
    V = hp.SquareMeshP1(-1.0, 1.0, nc)
    n, dt = V.nodes, 1e-3 * 80 / nc
    tl = (Nt + 1) * n
    rng = np.random.default_rng(nc)
    x, y = V.coordinates()
    prob = solvers.SolidBodyDrift(V, Nt, dt, batch=max(batches), order=hp.ORDER_VERTEX)
    o_all, o_3 = solvers.Observations.alltime(Nt, dt), solvers.Observations(Nt, [Nt // 4, Nt // 2, Nt])
    try:
        for B in batches:
            ctx = prob.ctx
            c = ctx.array(2.0 * rng.random(B * tl))
            u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
            u = ctx.array(np.tile(np.concatenate([u0, np.zeros(tl - n)]), B))
            prob.forward(c, u, batch=B)
            uh = ctx.array(0.9 * u.download() + 0.01)
            p = ctx.zeros(B * tl)
            t_a = median_ms(lambda: prob.adjoint(c, u, uh, p, "alltime", batch=B))
            t_oa = median_ms(lambda: prob.adjoint(c, u, uh, p, "snapshots", batch=B, obs=o_all))
            t_o3 = median_ms(lambda: prob.adjoint(c, u, uh, p, "snapshots", batch=B, obs=o_3))
            t_a2 = median_ms(lambda: prob.adjoint(c, u, uh, p, "alltime", batch=B))
            print(f"{nc + 1}^2 {B:3d}  {t_a:9.3f}  {t_a2:9.3f}  {t_oa:9.3f}  {t_o3:9.3f}  {t_a2 / t_a:.3f}  "
                  f"{t_oa / min(t_a, t_a2):.3f}  {t_o3 / min(t_a, t_a2):.3f}")
            for a in (c, u, uh, p):
                a.free()
    finally:
        prob.close()
