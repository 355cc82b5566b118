#!/usr/bin/env python3
"""Measurements of the control-zone primitives at config C2's size (81 x 81 P1 nodes, n = 6561, 251 time levels); writes
profiles/control_zones.txt.  Medians of --reps timed repetitions after --warmup untimed ones, a repetition = --inner calls
back to back closed by one device synchronise, the two sides of a comparison alternating repetition by repetition:

  kernels     femfct_zone_restrict without and with the mass rows, and femfct_zone_prolong with the inverse Gram matrix,
              on the 251 fields of a trajectory, for m = 4, 64 and 256 zones in a layout of blocks and a scattered one
              (label = node mod m).  Achieved bytes/s against the compulsory traffic: one read of the trajectory for a
              restriction, one write for a prolongation (the tables, the mass matrix and the m values per field are not
              counted, so a kernel that re-reads them looks the worse for it).
  direction   SolidBodyDrift.descent_direction with control_space= (right-hand side, restriction, m x m product,
              prolongation) against the free direction (right-hand side plus 251 Chebyshev mass solves of 20 iterations)

usage: python tools/bench_control_zones.py [--out profiles/control_zones.txt] [--reps 9] [--warmup 2] [--inner 50]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hp = importlib.import_module("fem-fct-pdeco_amd")
solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_zones.txt"))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--cells", type=int, default=80)
ap.add_argument("--steps", type=int, default=250)
args = ap.parse_args()

nc, Nt, dt = args.cells, args.steps, 1e-3
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
n, levels = mesh.nodes, Nt + 1
tl = levels * n
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX)
ctx = prob.ctx
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(*fns):
    """per call, (median, min, max) of every side, the sides alternating repetition by repetition"""
    for _ in range(args.warmup):
        for fn in fns:
            fn()
    ctx.synchronize()
    ts = {fn: [] for fn in fns}
    for _ in range(args.reps):
        for fn in fns:
            t = time.perf_counter()
            for _ in range(args.inner):
                fn()
            ctx.synchronize()
            ts[fn].append((time.perf_counter() - t) / args.inner)
    return [(float(np.median(v)), float(np.min(v)), float(np.max(v))) for v in ts.values()]


fmt = lambda t: f"{1e3 * t[0]:8.4f} [{1e3 * t[1]:.4f} .. {1e3 * t[2]:.4f}]"
gbs = lambda t: f"{8 * tl / t[0] / 1e9:7.1f} GB/s"
say(f"# control zones, n = {n}, {levels} levels, build {hp._lib.lib.femfct_build_id().decode()}")
say(f"# medians of {args.reps} repetitions of {args.inner} calls after {args.warmup} warm-ups (min .. max in brackets), "
    f"milliseconds per call; GB/s = {8 * tl / 1e6:.1f} MB (one pass over the trajectory) / median")

rng = np.random.default_rng(0)
x = ctx.array(rng.standard_normal(tl))
c, u, p = ctx.array(1.0 + rng.random(tl)), ctx.array(rng.random(tl)), ctx.array(0.05 * rng.standard_normal(tl))
d, rhs, s = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(levels * 256)
beta = 0.01


def layouts(m):
    b = int(round(np.sqrt(m)))
    return (("blocks", solvers.ControlZones.blocks(mesh, b, b, order=hp.ORDER_VERTEX)),
            ("scattered", solvers.ControlZones(np.arange(n) % m)))


free = lambda: prob.descent_direction(c, u, p, beta, d, scratch=rhs)
rhs_only = lambda: ctx.drift_gradient_rhs(c, u, p, beta, rhs, levels, prob.drift)
say()
for m in (4, 64, 256):
    for name, zones in layouts(m):
        Ginv = prob.zones_device(zones)
        plain = lambda: ctx.zone_restrict(x, levels, s)
        mass = lambda: ctx.zone_restrict(x, levels, s, apply_mass=True)
        prolong = lambda: ctx.zone_prolong(s, levels, d, Ginv=Ginv)
        tp, tm, tq = timed(plain, mass, prolong)
        say(f"m = {m:3d} {name:9s} zones of {int(zones.sizes.min())} .. {int(zones.sizes.max())} nodes, kappa(G) = "
            f"{np.linalg.cond(prob._zones_cache[id(zones)][2]):.2f}")
        say(f"    restrict          {fmt(tp)}  {gbs(tp)}")
        say(f"    restrict, mass    {fmt(tm)}  {gbs(tm)}")
        say(f"    prolong, Ginv     {fmt(tq)}  {gbs(tq)}")
        zoned = lambda: prob.descent_direction(c, u, p, beta, d, scratch=rhs, control_space=zones)
        tz, tf, tr = timed(zoned, free, rhs_only)
        say(f"    direction         zones {fmt(tz)}   free {fmt(tf)}   (right-hand side alone {fmt(tr)})   "
            f"zones / free = {tz[0] / tf[0]:.3f}")

prob.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
