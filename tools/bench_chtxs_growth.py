#!/usr/bin/env python3
"""Chemotaxis sweeps with and without the cell-growth term, on one context: graph replay, median of --reps sweeps after
warm-up, one process, forward (per-step control) and adjoint (all-time).  A step of the growth sweeps has the launches of
the growth-free one: k_chtxs_matrix_growth in the place of k_chtxs_matrix (forward) and of k_forms2 (adjoint).

usage: python tools/bench_chtxs_growth.py [--reps 30] > profiles/r07_chtxs_growth.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hp = importlib.import_module("fem-fct-pdeco_amd")
systems = importlib.import_module("fem-fct-pdeco_amd.systems")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()                     # a sweep returns after it has read its solver logs: synchronised
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


Nt, dt, growth, cpar = args.steps, 5e-4, (0.0, 1.0, -1.0), systems._chtxs_par()
print(f"# build {hp._lib.lib.femfct_build_id().decode()}: chemotaxis sweeps, {Nt} steps, growth {growth}, median of "
      f"{args.reps} sweeps after {args.warmup}; ms per sweep")
print("# nodes batch sweep  no_growth_ms  growth_ms  ratio")
for N, batches in ((41, (1, 20)), (129, (1,))):
    S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, N - 1), order=hp.ORDER_VERTEX)
    ctx, n = S.ctx, N * N
    tl = (Nt + 1) * n
    rng = np.random.default_rng(N)
    try:
        for B in batches:
            x0 = np.tile(np.concatenate([1.5 + 0.1 * (0.5 - rng.random(n)), np.zeros(tl - n)]), B)
            u, v, c = ctx.array(x0), ctx.array(x0), ctx.array(20 * rng.random(B * tl))
            uhat, vhat = ctx.array(1.4 + 0.1 * rng.random(B * tl)), ctx.array(1.6 + 0.1 * rng.random(B * tl))
            p, q = ctx.zeros(B * tl), ctx.zeros(B * tl)
            fwd = lambda g: ctx.chtxs_forward_ct(c, u, v, Nt, dt, cpar, 0.1, batch=B, growth=g)
            adj = lambda g: ctx.chtxs_adjoint(u, v, uhat, vhat, p, q, c, Nt, dt, cpar, 0.1, alltime=True, batch=B, growth=g)
            for name, fn in (("forward", fwd), ("adjoint", adj)):
                plain = median_ms(lambda: fn(None))
                grow = median_ms(lambda: fn(growth))
                print(f"{N}^2 {B:3d} {name}  {plain:9.3f}  {grow:9.3f}  {grow / plain:.3f}")
            for d in (u, v, c, uhat, vhat, p, q):
                d.free()
    finally:
        S.close()
