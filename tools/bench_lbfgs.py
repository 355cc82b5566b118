#!/usr/bin/env python3
"""The quasi-Newton primitives and loops at config C2's size (81 x 81 nodes, 250 steps, one trajectory of 13.2 MB):

  direction   femfct_free_set + femfct_q_gram + femfct_q_combine with J = 11 fields (a memory of 5), each alone and the
              three in sequence as LimitedMemory.direction issues them, beside one state sweep plus one adjoint sweep
  traffic     q_gram's least bytes (J trajectories and the mask read once) over its time, as a share of 8 TB/s
  descent     cost against sweeps on two all-time problems at this size (slotted disc and a smooth bump, target = the trajectory of c = 2,
              c0 = 1, beta = 1e-3, bounds [0, 5]) for lbfgs_solidbody with memory 0, 5, 8 and for pgd_solidbody_alltime

Times are the median over --reps of --calls back-to-back calls between two device synchronisations, divided by the
number of calls, after a warm-up (q_gram synchronises itself: its time includes the read-back of J*J doubles).

usage: python tools/bench_lbfgs.py [--reps 7] [--calls 10] [--iters 10] > profiles/r13_lbfgs.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
hp = importlib.import_module("fem-fct-pdeco_amd")
solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
from _common import slotted_disc, to_dof

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--iters", type=int, default=10)
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


nc, Nt, dt, J = 80, 250, 1e-3, 11
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX)
ctx, n, tl = prob.ctx, prob.n, prob.tlen
print(f"# build {hp._lib.lib.femfct_build_id().decode()}: n = {n}, {Nt + 1} levels, trajectory {8 * tl / 1e6:.2f} MB; median of "
      f"{args.reps} x ({args.calls} calls between two synchronisations) / {args.calls}")
rng = np.random.default_rng(13)
fields = [ctx.array(rng.standard_normal(tl)) for _ in range(J)]
c = ctx.array(rng.uniform(-0.5, 5.5, tl).clip(0.0, 5.0))
out, mask = ctx.empty(tl), ctx.empty((tl + 7) // 8)
coef = rng.standard_normal(J)
g = fields[-1]
t_free = timed(ctx, lambda: ctx.free_set(c, g, 0.0, 5.0, tl, mask))
t_comb = timed(ctx, lambda: ctx.q_combine(fields, coef, tl, out, mask=mask, fallback=g, fallback_scale=-1.0))
print("\n## direction: microseconds per call")
print(f"free_set                        {t_free:10.1f}")
for JJ in (1, 2, 11, 17):
    ff = (fields + fields)[:JJ]
    t_m = timed(ctx, lambda: ctx.q_gram(ff, Nt, dt, mask=mask))
    t_u = timed(ctx, lambda: ctx.q_gram(ff, Nt, dt))
    bytes_m, bytes_u = JJ * 8 * tl + tl, JJ * 8 * tl
    print(f"q_gram J = {JJ:2d}   masked {t_m:10.1f}  ({bytes_m / 1e6:7.2f} MB, {bytes_m / t_m / 1e6 / 8.0 * 100:5.2f} % of 8 TB/s)   "
          f"unmasked {t_u:10.1f}  ({bytes_u / t_u / 1e6 / 8.0 * 100:5.2f} %)")
print(f"q_combine J = {J}                {t_comb:10.1f}")


def direction():
    ctx.free_set(c, g, 0.0, 5.0, tl, mask)
    G = ctx.q_gram(fields, Nt, dt, mask=mask)
    ctx.q_combine(fields, coef, tl, out, mask=mask, fallback=g, fallback_scale=-1.0)
    return G


t_dir = timed(ctx, direction)
t_norm = timed(ctx, lambda: ctx.l2_norm_sq_Q(g, None, Nt, dt))
u, p, uh = ctx.zeros(tl), ctx.zeros(tl), ctx.array(rng.random(tl))
cc = ctx.array(np.full(tl, 1.5))
u.upload(np.concatenate([rng.random(n), np.zeros(tl - n)]))
t_fwd = timed(ctx, lambda: prob.forward(cc, u, batch=1))
t_adj = timed(ctx, lambda: prob.adjoint(cc, u, uh, p, "alltime", batch=1))
print(f"free_set + q_gram + q_combine   {t_dir:10.1f}   (J = {J}, in sequence)")
print(f"l2_norm_sq_Q of one trajectory  {t_norm:10.1f}   (the only L2(Q) reduction before)")
print(f"state sweep + adjoint sweep     {t_fwd + t_adj:10.1f}   ({t_fwd:.1f} + {t_adj:.1f}; {Nt} steps each)")
print(f"direction / (state + adjoint)   {t_dir / (t_fwd + t_adj):10.4f}")

# ---- cost against sweeps
dx = 2.0 / nc
x, y = mesh.coordinates()
c0, beta, lo, hi = np.ones(tl), 1e-3, 0.0, 5.0
problems = (("slotted disc (C2's initial condition)",
             hp.reorder_vector_from_dof(to_dof(mesh, slotted_disc(-1.0, 1.0, dx)), 1, n, mesh.vertex_to_dof)),
            ("smooth bump exp(-15((x+0.2)^2+(y-0.1)^2)) (the tests' initial condition)",
             np.exp(-15 * ((x + 0.2) ** 2 + (y - 0.1) ** 2))))
for label, u0 in problems:
    uhat = np.zeros(tl)
    uhat[:n] = u0
    prob.solve_state(np.full(tl, 2.0), uhat)
    print(f"\n## descent, {label}: all-time tracking of the trajectory of c = 2 from c0 = 1, beta = {beta}, bounds "
          f"[{lo}, {hi}], {args.iters} iterations")
    print("# sweeps = state and adjoint sweeps a sequential search runs (trials are evaluated as one batch of 10); k = trials looked at")
    runs = {}
    for mem in (0, 5, 8):
        t0 = time.perf_counter()
        h = solvers.lbfgs_solidbody(prob, u0, uhat, c0, beta, lo, hi, args.iters, memory=mem, optim="alltime")[3]
        runs[f"lbfgs m={mem}"] = (h["sweeps"], h["cost"], h["armijo_k"], time.perf_counter() - t0, h)
    t0 = time.perf_counter()
    h = solvers.pgd_solidbody_alltime(prob, u0, uhat, c0, beta, lo, hi, args.iters)[3]
    # the reference loop: per iteration one adjoint sweep, the state of the unconditional first step, one state per trial
    runs["pgd_alltime"] = (list(np.cumsum([2 + k for k in h["armijo_k"]])), h["cost"], h["armijo_k"], time.perf_counter() - t0, h)
    print(f"# J(c0) = {runs['lbfgs m=0'][4]['cost0']:.6e}")
    print("# it   " + "   ".join(f"{name:>24s}" for name in runs))
    print("#      " + "   ".join(f"{'sweeps  J           k':>24s}" for _ in runs))
    for k in range(args.iters):
        row = []
        for name, (sw, cost, ak, _, _) in runs.items():
            row.append(f"{sw[k]:6d}  {cost[k]:.4e}  {ak[k]:2d}".rjust(24) if k < len(cost) else " " * 24)
        print(f"  {k + 1:3d}   " + "   ".join(row))
    for name, (_, _, _, el, h) in runs.items():
        extra = "" if "used" not in h else (f"  used {''.join('q' if v == 'qn' else 'g' for v in h['used'])}  free_min "
                                            f"{min(h['free_fraction']):.3f}  stalled {h['stalled']}")
        print(f"# {name}: {el:.2f} s wall{extra}")
prob.close()
