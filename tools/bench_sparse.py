#!/usr/bin/env python3
"""The primitives of the L1-sparse control loops at config C2's size (81 x 81 nodes, 251 levels, one trajectory of
13.2 MB, K = 10 trials):

  prox_trials          femfct_prox_trials without and with sources, beside femfct_source_trials (the kernel of the same
                       traffic before) at the same K
  l1_norm_Q            of one trajectory and of the K trials
  sparse_trial_stats   the fused pass, beside the three calls it replaces in the same process: K device copies of c, then
                       l2_norm_sq_Q(c_t - c) with batch K, then l1_norm_Q with batch K (which leaves out the count)

Times are the median over --reps of --calls back-to-back calls between two device synchronisations, divided by the
number of calls, after a warm-up (the reductions synchronise themselves: their times include the read-back).  The whole
measurement is repeated --rounds times: the spread of the repeated medians is what a difference has to beat.  Least
bytes: every input read once and every output written once.

usage: python tools/bench_sparse.py [--reps 7] [--calls 10] [--rounds 3] > profiles/sparse_controls.txt"""
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
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
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


nc, Nt, dt, K = 80, 250, 1e-3, 10
alpha, lo, hi = 0.3, -0.1, 0.5       # a third of the first trial's values are exactly zero, fewer as the step halves
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX)
ctx, n, tl = prob.ctx, prob.n, prob.tlen
MB = 8 * tl / 1e6
print(f"# build {hp._lib.lib.femfct_build_id().decode()}: n = {n}, {Nt + 1} levels, trajectory {MB:.2f} MB, K = {K}; median of "
      f"{args.reps} x ({args.calls} calls between two synchronisations) / {args.calls}, {args.rounds} rounds")
rng = np.random.default_rng(17)
c, d, g = ctx.array(rng.uniform(-0.3, 0.7, tl)), ctx.array(0.3 * rng.standard_normal(tl)), ctx.array(rng.standard_normal(tl))
cB, srcB, ckB = ctx.empty(K * tl), ctx.empty(K * tl), ctx.empty(K * tl)
ctx.prox_trials(c, d, 1.0, K, alpha, lo, hi, tl, cB)


def copies():
    for k in range(K):
        ckB.copy_from(c, tl, dst_off=k * tl)


def trio():
    copies()
    dist = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=K)
    return ctx.l1_norm_Q(cB, Nt, dt, batch=K), dist


cases = (
    ("prox_trials, no sources", lambda: ctx.prox_trials(c, d, 1.0, K, alpha, lo, hi, tl, cB), (2 + K) * MB),
    ("source_trials, no sources", lambda: ctx.source_trials(c, d, 1.0, K, lo, hi, tl, ckB), (2 + K) * MB),
    ("prox_trials, g and sources", lambda: ctx.prox_trials(c, d, 1.0, K, alpha, lo, hi, tl, ckB, srcB, g=g), (3 + 2 * K) * MB),
    ("source_trials, g and sources", lambda: ctx.source_trials(c, d, 1.0, K, lo, hi, tl, ckB, srcB, g=g), (3 + 2 * K) * MB),
    ("l1_norm_Q, one trajectory", lambda: ctx.l1_norm_Q(c, Nt, dt), MB),
    ("l1_norm_Q, batch K", lambda: ctx.l1_norm_Q(cB, Nt, dt, batch=K), K * MB),
    ("sparse_trial_stats (fused)", lambda: ctx.sparse_trial_stats(cB, c, K, Nt, dt), (K + 1) * MB),
    ("unfused: K copies of c", copies, 2 * K * MB),
    ("unfused: l2_norm_sq_Q batch K", lambda: ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=K), 2 * K * MB),
    ("unfused trio (copies, l2, l1)", trio, 5 * K * MB),
)
rows = {name: [] for name, _, _ in cases}
for _ in range(args.rounds):
    for name, fn, _ in cases:
        rows[name].append(timed(ctx, fn))
print("\n## microseconds per call (median of the rounds; every round), least bytes, share of 8 TB/s")
for name, _, mb in cases:
    t = float(np.median(rows[name]))
    print(f"{name:32s} {t:10.1f}   ({'  '.join(f'{v:9.1f}' for v in rows[name])})   {mb:8.2f} MB   {mb / t / 8.0 * 100:6.2f} %")
f, u = np.array(rows["sparse_trial_stats (fused)"]), np.array(rows["unfused trio (copies, l2, l1)"])
p, s = np.array(rows["prox_trials, no sources"]), np.array(rows["source_trials, no sources"])
print(f"\nprox_trials / source_trials (no sources)      {np.median(p) / np.median(s):.3f}")
print(f"fused statistics / unfused trio               {np.median(f) / np.median(u):.3f}   "
      f"(fused {f.min():.1f}..{f.max():.1f} us, trio {u.min():.1f}..{u.max():.1f} us over the rounds)")
print("fused beats the trio by more than the spread of the repeated medians: "
      f"{'yes' if f.max() < u.min() and u.min() - f.max() > max(np.ptp(f), np.ptp(u)) else 'no'}")
l1, dist, nnz = ctx.sparse_trial_stats(cB, c, K, Nt, dt)
l1u, distu = trio()
print(f"fused == unfused bit for bit: l1 {l1.tobytes() == l1u.tobytes()}, dist {dist.tobytes() == distu.tobytes()}; "
      f"nonzero share of the trials {nnz[0] / tl:.3f} .. {nnz[-1] / tl:.3f}")
prob.close()
