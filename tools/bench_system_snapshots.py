#!/usr/bin/env python3
"""Adjoint sweeps of the three PDE systems with snapshot observations against their all-time sweeps on the same inputs:
graph replay, median of --reps 40-step sweeps after warm-up, every timing on a context of its own, so that each sees the
same history of its context (the Chebyshev species budget of the Schnakenberg adjoint at 129^2 grows with every sweep of a
context, whatever its misfit: DESIGN.md section 2).  A snapshot step has the launches of the
all-time step, with the k_*_obs kernels in the place of the load launches.

  alltime_ms / alltime2_ms   the system's all-time adjoint, timed on two fresh contexts: their ratio is the spread of a
                             repeated run on the box, the yardstick for the other ratios
  parent_ms                  the all-time adjoint of another checkout of this repository (--parent-tree, e.g. the parent
                             commit's, built), timed by a fresh child process on the same inputs ("-": not given)
  obs_all_ms                 observations at every level (Observations.alltime; chemotaxis: once per load, "nodal" is the
                             all-time sweep's arithmetic)
  obs_2_ms                   two observed levels (Nt/2 and Nt): the other levels' loads read no target
  ratios                     obs_all and obs_2 against the parent's all-time sweep (this build's where no parent is given)

usage: python tools/bench_system_snapshots.py [--reps 30] [--parent-tree PATH] > profiles/r10_system_snapshots.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--parent-tree", default=None, help="another built checkout whose all-time sweeps are timed for comparison")
ap.add_argument("--alltime-only", action="store_true", help="time the all-time sweeps alone and print them as JSON")
ap.add_argument("--root", default=ROOT, help="the checkout whose package and library run (default: this file's)")
args = ap.parse_args()

parent = {}
if args.parent_tree and not args.alltime_only:      # before this process opens the GPU: a fresh child with the other checkout
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--alltime-only", "--root", os.path.abspath(args.parent_tree),
                          "--reps", str(args.reps), "--warmup", str(args.warmup)], capture_output=True, text=True, check=True)
    parent = json.loads(out.stdout.strip().splitlines()[-1])

sys.path.insert(0, args.root)
import importlib  # noqa: E402
hp = importlib.import_module("fem-fct-pdeco_amd")
systems = importlib.import_module("fem-fct-pdeco_amd.systems")
solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
DeviceObs = getattr(importlib.import_module("fem-fct-pdeco_amd.device"), "DeviceObs", None)     # (absent in an older checkout)
hp.fct_helpers.VERBOSE = False

Nt = 40
DT = {"nonlinear": 1e-3, "schnak": 5e-4, "chtxs": 5e-4}


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()                     # a sweep returns after it has read its solver log: synchronised
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def setup(S, system, B, rng):
    """states by the device's forward sweep (per-step control), targets next to them; returns sweep(obs, misfit)"""
    kw = lambda obs, misfit=None: {} if obs is None else (dict(obs=obs) if misfit is None else dict(obs=obs, misfit=misfit))
    ctx, n = S.ctx, S.n
    tl = (Nt + 1) * n
    dt = DT[system]
    x, y = S.mesh.coordinates()
    z = lambda x0: np.tile(np.concatenate([x0, np.zeros(tl - n)]), B)
    if system == "nonlinear":
        eps, _, wind = systems.get_nonlinear_eqns_params()
        Aw, _ = S.convection(wind, "nonlinear")
        u = ctx.array(z(5 * y * (y - 1) * x * (x - 1) * np.sin(4 * np.pi * x)))
        ctx.nonlinear_forward_ct(Aw, ctx.array(rng.random(B * tl)), u, Nt, dt, eps, batch=B)
        uh, p = ctx.array(0.8 * u.download() + 0.05 * rng.random(B * tl)), ctx.zeros(B * tl)
        return lambda obs=None, misfit="mass": ctx.nonlinear_adjoint(Aw, u, uh, p, Nt, dt, eps, batch=B, alltime=True, **kw(obs))
    if system == "schnak":
        par, wind = systems._schnak_par()
        Aw, AwT = S.convection(wind, "schnak")
        u, v = ctx.array(z(1.0 + 0.1 * np.cos(2 * np.pi * (x + y)))), ctx.array(z(0.9 + 0.1 * np.cos(2 * np.pi * (x - y))))
        ctx.schnak_forward_ct(Aw, ctx.array(0.1 + 0.05 * rng.random(B * tl)), u, v, Nt, dt, par, 1.0, batch=B)
        uh, vh = ctx.array(0.9 * u.download() + 0.02 * rng.random(B * tl)), ctx.array(1.1 * v.download() + 0.02 * rng.random(B * tl))
        p, q = ctx.zeros(B * tl), ctx.zeros(B * tl)
        return lambda obs=None, misfit="mass": ctx.schnak_adjoint(AwT, u, v, uh, vh, p, q, Nt, dt, par, batch=B, alltime=True, **kw(obs))
    cpar = systems._chtxs_par()
    u0 = 1.5 + 0.1 * (0.5 - rng.random(n))
    u, v, c = ctx.array(z(u0)), ctx.array(z(u0)), ctx.array(20 * rng.random(B * tl))
    ctx.chtxs_forward_ct(c, u, v, Nt, dt, cpar, 0.1, batch=B, growth=(0.0, 1.0, -1.0))
    uh, vh = ctx.array(0.9 * u.download() + 0.02 * rng.random(B * tl)), ctx.array(1.05 * v.download() + 0.02 * rng.random(B * tl))
    p, q = ctx.zeros(B * tl), ctx.zeros(B * tl)
    return lambda obs=None, misfit="mass": ctx.chtxs_adjoint(u, v, uh, vh, p, q, c, Nt, dt, cpar, 0.1, alltime=True, batch=B,
                                                             growth=(0.0, 1.0, -1.0), **kw(obs, misfit))


if not args.alltime_only:
    print(f"# build {hp._lib.lib.femfct_build_id().decode()}: adjoint sweeps of the PDE systems, {Nt} steps, median of {args.reps} "
          f"sweeps after {args.warmup}; ms per sweep; chemotaxis with growth (0, 1, -1)"
          + (f"; parent_ms: all-time sweep of build {parent.get('build', '?')}" if parent else ""))
    print("# system       nodes batch  alltime_ms  alltime2_ms  parent_ms  obs_all_ms  obs_2_ms  spread  obs_all/ref  obs_2/ref")
times = {"build": hp._lib.lib.femfct_build_id().decode()}


def timed(V, system, N, B, mode, misfit="mass"):
    """median ms of one mode on a context of its own: every timing sees the same history of its context"""
    S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
    try:
        sweep = setup(S, system, B, np.random.default_rng([N, B]))
        if mode == "alltime":
            return median_ms(sweep)
        dt = DT[system]
        o = solvers.Observations.alltime(Nt, dt) if mode == "obs_all" else solvers.Observations(Nt, [Nt // 2, Nt])
        dev = DeviceObs(S.ctx.array(o.theta), o.tau, S.ctx.array(o.theta) if system != "nonlinear" else None, o.tau)
        return median_ms(lambda: sweep(dev, misfit))
    finally:
        S.close()


for N, batches in ((41, (1, 20)), (129, (1,))):
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    for system in ("nonlinear", "schnak", "chtxs"):
        for B in batches:
            t_a = timed(V, system, N, B, "alltime")
            if args.alltime_only:
                times[f"{system}/{N}/{B}"] = t_a
                continue
            rows = [("nodal", "chtxs-nodal"), ("mass", "chtxs-mass")] if system == "chtxs" else [("mass", system)]
            res = [(name, timed(V, system, N, B, "obs_all", mf), timed(V, system, N, B, "obs_2", mf)) for mf, name in rows]
            t_a2 = timed(V, system, N, B, "alltime")
            t_p = parent.get(f"{system}/{N}/{B}")
            ref = t_p if t_p is not None else min(t_a, t_a2)
            for name, t_oa, t_o2 in res:
                print(f"{name:12s} {N}^2 {B:3d}  {t_a:9.3f}  {t_a2:9.3f}  {'-' if t_p is None else format(t_p, '9.3f')}  {t_oa:9.3f}  "
                      f"{t_o2:9.3f}  {t_a2 / t_a:.3f}  {t_oa / ref:.3f}  {t_o2 / ref:.3f}")
if args.alltime_only:
    print(json.dumps(times))
