#!/usr/bin/env python3
"""Measurements of the smooth-control primitives at config C2's size (81 x 81 P1 nodes, n = 6561) with the step count of
examples/smooth_control_pdeco.py (100 steps of 1e-3, 101 levels); writes profiles/smooth_controls.txt.  Medians of --reps
timed repetitions after --warmup untimed ones, a repetition being --inner calls back to back closed by one device
synchronise, --rounds alternating rounds in one process, every round printed:

  smooth_cost   femfct_smooth_cost at batch 1 and at the loops' max_armijo (10): one pass over c, one read-back per call
  smooth_rhs    femfct_smooth_rhs, one trajectory
  fused         femfct_drift_gradient_rhs_smooth against femfct_drift_gradient_rhs on the same inputs (the parent commit's
                kernel: profiles/kernel_fingerprints.txt shows its machine code unchanged) and against the unfused
                sequence drift_gradient_rhs + smooth_rhs + axpby that gives the same bits
  direction     SolidBodyDrift.descent_direction (the right-hand side and the num_steps + 1 mass solves) without and with
                the term: what the fused launch's extra time is a share of

Each result is also given as the rate of its compulsory bytes (every input trajectory read once, the output stored once)
and that rate's share of 8 TB/s.  At this size every trajectory (5.3 MB) sits in cache: the shares say how far a call is
from the HBM roofline a large mesh would meet, not what HBM delivered.

usage: python tools/bench_smoothness.py [--out profiles/smooth_controls.txt] [--reps 7] [--warmup 2] [--inner 20]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_controls.txt"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cells", type=int, default=80)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--trials", type=int, default=10)
args = ap.parse_args()

nc, Nt, dt, K = args.cells, args.steps, 1e-3, args.trials
beta, bx, bt = 0.05, 5e-5, 1e-7
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
n, levels = mesh.nodes, Nt + 1
tl = levels * n
x, y = mesh.coordinates()
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX)
ctx = prob.ctx
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def median_time(fn):
    for _ in range(args.warmup):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        for _ in range(args.inner):
            fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t) / args.inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


t = np.arange(levels)[:, None] * dt
rng = np.random.default_rng(0)
c = ctx.array((0.5 + 0.3 * np.sin(6 * x)[None] * np.cos(5 * y)[None] * np.cos(0.8 / dt * t)).ravel())
cB = ctx.array(np.tile(c.download(), K) + 0.01 * rng.random(K * tl))
u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
u, p = ctx.zeros(tl), ctx.zeros(tl)
u.upload(np.concatenate([u0, np.zeros(tl - n)]))
prob.forward(c, u, batch=1)
uhT = ctx.array(0.9 * u.download()[Nt * n:])
prob.adjoint(c, u, uhT, p, "finaltime", batch=1)
a, b, s, f = ctx.empty(tl), ctx.empty(tl), ctx.empty(tl), ctx.empty(tl)
sm = solvers.Smoothness(bx, bt)

ctx.drift_gradient_rhs(c, u, p, beta, a, levels, prob.drift)
ctx.smooth_rhs(c, bx, bt, Nt, dt, b)
ctx.axpby(tl, 1.0, a, 1.0, b, s)
ctx.drift_gradient_rhs_smooth(c, u, p, beta, bx, bt, dt, f, levels, prob.drift)
same = np.array_equal(f.download().view(np.int64), s.download().view(np.int64))

cases = [
    ("smooth_cost batch 1", lambda: ctx.smooth_cost(c, Nt, dt), 1 * tl),
    (f"smooth_cost batch {K}", lambda: ctx.smooth_cost(cB, Nt, dt, batch=K), K * tl),
    ("smooth_rhs", lambda: ctx.smooth_rhs(c, bx, bt, Nt, dt, b), 2 * tl),
    ("drift_gradient_rhs (parent's kernel)", lambda: ctx.drift_gradient_rhs(c, u, p, beta, a, levels, prob.drift), 4 * tl),
    ("drift_gradient_rhs_smooth (fused)", lambda: ctx.drift_gradient_rhs_smooth(c, u, p, beta, bx, bt, dt, f, levels, prob.drift),
     4 * tl),
    ("drift_gradient_rhs + smooth_rhs + axpby", lambda: (ctx.drift_gradient_rhs(c, u, p, beta, a, levels, prob.drift),
                                                         ctx.smooth_rhs(c, bx, bt, Nt, dt, b),
                                                         ctx.axpby(tl, 1.0, a, 1.0, b, s)), 9 * tl),
    ("descent_direction", lambda: prob.descent_direction(c, u, p, beta, s, scratch=a), None),
    ("descent_direction(smoothness)", lambda: prob.descent_direction(c, u, p, beta, s, scratch=a, smoothness=sm), None),
]

say(f"# smooth controls, n = {n}, {levels} levels ({8 * tl / 1e6:.2f} MB a trajectory), beta_x = {bx:g}, beta_t = {bt:g}, "
    f"build {hp._lib.lib.femfct_build_id().decode()}")
say(f"# microseconds per call: median of {args.reps} repetitions of {args.inner} calls and one synchronise, after {args.warmup} "
    f"warm-ups [min .. max]; compulsory bytes, their rate and its share of 8 TB/s")
say(f"# fused output equals drift_gradient_rhs + smooth_rhs (axpby) bit for bit: {same}")
med = {}
for r in range(args.rounds):
    say(f"round {r + 1}")
    for name, fn, doubles in cases:
        m, lo, hi = median_time(fn)
        med.setdefault(name, []).append(m)
        line = f"  {name:42s} {1e6 * m:9.2f} [{1e6 * lo:.2f} .. {1e6 * hi:.2f}] us"
        if doubles is not None:
            byts = 8 * doubles
            line += f"   {byts / 1e6:7.2f} MB   {byts / m / 1e12:6.3f} TB/s   {byts / m / 8e12:6.3f}"
        say(line)
best = {k: float(np.median(v)) for k, v in med.items()}
spread = max(max(v) / min(v) for v in med.values())
fused, parent, seq = (best[cases[i][0]] for i in (4, 3, 5))
say(f"# medians over the rounds: fused {1e6 * fused:.2f} us = {fused / parent:.3f} x the parent's kernel, "
    f"{fused / seq:.3f} x the unfused sequence; a direction with the term {best[cases[7][0]] / best[cases[6][0]]:.3f} x one "
    f"without; largest max / min of a case's round medians {spread:.3f}")
prob.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
