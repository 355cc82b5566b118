#!/usr/bin/env python3
"""Times of the time restriction / prolongation of piecewise-constant controls (femfct_time_restrict, femfct_time_prolong)
and of the projected descent direction of the drift-control problem, at the sizes of config C2 (81 x 81 nodes, 250 steps)
and config C3 (41 x 41 nodes, 200 steps), one trajectory:

  kernels     time_restrict and time_prolong alone, K in {1, 5, Nt + 1}
  direction   SolidBodyDrift.descent_direction(control_time=ControlIntervals) with K in {1, 5, Nt + 1}: the gradient
              right-hand sides of all levels, restrict, K mass solves (ChebSI, 20 iterations), prolong
  free        the same call with control_time=None: Nt + 1 mass solves, the comparison

Each figure is the median over --reps of the time of --calls back-to-back calls between two device synchronisations,
divided by the number of calls, after a warm-up.  At these sizes the trajectories sit in cache (13 MB and 2.7 MB), so the
table gives times and the bytes each call moves at least, and no share of a memory roofline.

usage: python tools/bench_control_intervals.py [--reps 7] [--calls 20] > profiles/r12_control_intervals.txt"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()


def timed(ctx, fn):
    """median microseconds per call"""
    for _ in range(3):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) / args.calls)
    return 1e6 * float(np.median(ts))


print(f"# build {hp._lib.lib.femfct_build_id().decode()}: median of {args.reps} x ({args.calls} calls between two "
      f"synchronisations) / {args.calls}, microseconds per call; one trajectory; bytes = least traffic of the call")
for name, nc, Nt, dt in (("C2", 80, 250, 1e-3), ("C3", 40, 200, 5e-4)):
    mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
    prob = solvers.SolidBodyDrift(mesh, Nt, dt, order=hp.ORDER_VERTEX)
    ctx, n, tl = prob.ctx, prob.n, prob.tlen
    rng = np.random.default_rng(12)
    c, u, p = (ctx.array(rng.standard_normal(tl)) for _ in range(3))
    d, rhs = ctx.zeros(tl), ctx.empty(tl)
    print(f"\n## {name}'s size: n = {n}, {Nt + 1} levels, trajectory {8 * tl / 1e6:.2f} MB")
    print("# K      restrict_us   restrict_MB   prolong_us   prolong_MB   direction_us")
    for K in (1, 5, Nt + 1):
        if K == 1:
            ct = solvers.ControlIntervals.stationary(Nt)
        elif K == Nt + 1:
            ct = solvers.ControlIntervals.identity(Nt)
        else:
            ct = solvers.ControlIntervals.every(Nt, -(-(Nt + 1) // K))
        assert ct.K == K, (ct.K, K)
        yk = ctx.zeros(K * n)
        chunks = sum(-(-int(L) // 32) for L in np.diff(ct.starts) if L > 32)       # partials written and read back
        t_r = timed(ctx, lambda: ctx.time_restrict(u, ct.starts, Nt, yk))
        t_p = timed(ctx, lambda: ctx.time_prolong(yk, ct.starts, Nt, d))
        t_d = timed(ctx, lambda: prob.descent_direction(c, u, p, 0.01, d, scratch=rhs, control_time=ct))
        print(f"  {K:4d}   {t_r:10.2f}   {8 * (tl + K * n + 2 * chunks * n) / 1e6:10.3f}   {t_p:10.2f}   "
              f"{8 * (K * n + tl) / 1e6:10.3f}   {t_d:12.2f}")
        yk.free()
    t_f = timed(ctx, lambda: prob.descent_direction(c, u, p, 0.01, d, scratch=rhs))
    t_g = timed(ctx, lambda: ctx.drift_gradient_rhs(c, u, p, 0.01, rhs, Nt + 1, prob.drift))
    print(f"# control_time=None (the free control: {Nt + 1} mass solves)   direction_us {t_f:12.2f}")
    print(f"# drift_gradient_rhs alone (part of every direction above)        {t_g:12.2f}")
    prob.close()
