#!/usr/bin/env python3
"""State sweep of the linear source-control problem with and without the reaction term, on one context: graph replay,
median of --reps sweeps after warm-up, one process.  The step of the reaction sweep has the same launches, with
k_react_load in the place of k_mass_diff.

usage: python tools/bench_reaction_source.py [--reps 30] > profiles/r06_reaction_source.txt"""
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


print(f"# build {hp._lib.lib.femfct_build_id().decode()}: state sweep, 40 steps, median of {args.reps} sweeps after "
      f"{args.warmup}; ms per sweep")
print("# nodes order batch  no_reaction_ms  reaction_ms  ratio")
Nt, eps = 40, 1e-4
wind = solvers.finaltime_exact_wind()
for nc, order, batches in ((20, hp.ORDER_FENICS, (1, 10)), (20, hp.ORDER_VERTEX, (1, 10)), (80, hp.ORDER_VERTEX, (1, 10))):
    V = hp.SquareMeshP1(0.0, 1.0, nc)
    n, dt = V.nodes, (1.0 / nc) ** 2
    tl = (Nt + 1) * n
    rng = np.random.default_rng(nc)
    g = -55.0 + 45.0 * rng.random(tl)
    prob = solvers.LinearReactionSourceControl(V, Nt, dt, wind, g, eps=eps, batch=max(batches), order=order)
    try:
        for B in batches:
            src = prob.ctx.array(rng.standard_normal(B * tl))
            u = prob.ctx.array(np.tile(np.concatenate([1.0 + rng.random(n), np.zeros(tl - n)]), B))
            plain = median_ms(lambda: solvers.LinearSourceControl.state(prob, src, u, batch=B))
            react = median_ms(lambda: prob.state(src, u, batch=B))
            print(f"{nc + 1}^2 {'vertex' if order == hp.ORDER_VERTEX else 'fenics'} {B:3d}  {plain:9.3f}  {react:9.3f}  "
                  f"{react / plain:.3f}")
            src.free()
            u.free()
    finally:
        prob.close()
