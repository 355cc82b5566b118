#!/usr/bin/env python3
"""Measurements of the initial-state recovery at config C2's size (81 x 81 P1 nodes, n = 6561, 250 steps of 1e-3, K = 10
trials); writes profiles/initial_state.txt.  Medians of --reps timed repetitions after --warmup untimed ones, every timed
region closed by a device synchronise, the two sides of a comparison alternating repetition by repetition in one process:

  trials+stats  femfct_initial_trials + femfct_initial_trial_stats against the sequence of existing entry points they
                replace: femfct_trial_controls into a staging buffer, K device copies into level 0 of the batch, 2K
                femfct_l2_norm_sq_Omega calls
  gram          femfct_omega_gram with J = 7 fields (a memory of 3) against J (J + 1) / 2 femfct_l2_norm_sq_Omega calls
  iteration     one iteration of solvers.initial_state_solidbody (final-time, memory 3), speculative and sequential: the
                time between the accepted steps of --iters iterations, with the trials each looked at

usage: python tools/bench_initial_state.py [--out profiles/initial_state.txt] [--reps 9] [--warmup 2] [--iters 4]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initial_state.txt"))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--cells", type=int, default=80)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--trials", type=int, default=10)
args = ap.parse_args()

nc, Nt, dt, K = args.cells, args.steps, 1e-3, args.trials
beta0, lo, hi = 1e-3, 0.0, 0.8
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
n = mesh.nodes
tl = (Nt + 1) * n
x, y = mesh.coordinates()
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX, batch=K)
ctx = prob.ctx
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def compare(new, old, inner=5):
    """per call, (median, min, max) of each side: a repetition is ``inner`` calls back to back and one synchronise, the
    sides alternating"""
    for _ in range(args.warmup):
        new(), old()
    ctx.synchronize()
    ts = {new: [], old: []}
    for _ in range(args.reps):
        for fn in (new, old):
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.synchronize()
            ts[fn].append((time.perf_counter() - t) / inner)
    return tuple((float(np.median(v)), float(np.min(v)), float(np.max(v))) for v in (ts[new], ts[old]))


fmt = lambda t: f"{1e3 * t[0]:8.3f} [{1e3 * t[1]:.3f} .. {1e3 * t[2]:.3f}]"
say(f"# initial-state recovery, n = {n}, {Nt} steps, K = {K} trials, build {hp._lib.lib.femfct_build_id().decode()}")
say(f"# medians of {args.reps} repetitions after {args.warmup} warm-ups (min .. max in brackets), milliseconds per call")
say(f"# sweep kernels: regime {ctx.kernel_regime(K)} at batch {K}, {ctx.kernel_regime(1)} at batch 1")

rng = np.random.default_rng(0)
truth = np.exp(-15 * ((x + 0.2) ** 2 + (y - 0.1) ** 2))
v0 = np.exp(-15 * ((x - 0.1) ** 2 + (y + 0.2) ** 2))
v, vb, d = ctx.array(v0), ctx.array(0.5 * v0), ctx.array(truth - v0)
steps = 4.0 * (1 / 2 ** np.arange(K))
uB, stage = ctx.zeros(K * tl), ctx.empty(K * n)


def new_trials():
    ctx.initial_trials(v, d, steps, lo, hi, uB, Nt)
    return ctx.initial_trial_stats(uB, v, K, Nt, vb=vb)


def old_trials():
    ctx.trial_controls(v, d, steps, 1, K, lo, hi, n, stage)
    for k in range(K):
        uB.copy_from(stage, n, dst_off=k * tl, src_off=k * n)
    return np.array([[ctx.l2_norm_sq_Omega(uB.ptr + 8 * k * tl, vb)[0], ctx.l2_norm_sq_Omega(uB.ptr + 8 * k * tl, v)[0]]
                     for k in range(K)])


assert new_trials().tobytes() == old_trials().tobytes()          # the same bits, so the same work
t_new, t_old = compare(new_trials, old_trials)
say()
say(f"trials+stats  initial_trials + initial_trial_stats {fmt(t_new)}   (2 launches + 1 fold, 1 read-back)")
say(f"              trial_controls + {K} copies + {2 * K} x l2_norm_sq_Omega {fmt(t_old)}   "
    f"({1 + 5 * K} launches and copies, {2 * K} read-backs)   ratio {t_old[0] / t_new[0]:.2f}")

J = 7
fields = [ctx.array(rng.standard_normal(n)) for _ in range(J)]
new_gram = lambda: ctx.omega_gram(fields)
old_gram = lambda: [ctx.l2_norm_sq_Omega(fields[i], None if i == j else fields[j]) for j in range(J) for i in range(j + 1)]
t_new, t_old = compare(new_gram, old_gram)
say(f"gram J = {J}    omega_gram {fmt(t_new)}   (1 launch + 1 fold, 1 read-back)")
say(f"              {J * (J + 1) // 2} x l2_norm_sq_Omega {fmt(t_old)}   ratio {t_old[0] / t_new[0]:.2f}")

# -- one whole iteration
c = np.full(tl, 2.0)
traj = ctx.zeros(tl)
traj.copy_from(ctx.array(truth), n)
cd = ctx.array(c)
prob.forward(cd, traj, batch=1)
uhat_T = traj.download()[Nt * n:].copy()


def run(speculative):
    h = solvers.initial_state_solidbody(prob, c, uhat_T, v0, beta0, lo, hi, args.iters, background=0.5 * v0, memory=3,
                                        s0=4.0, max_armijo=K, speculative=speculative)[3]
    return np.diff([h["wall0"]] + h["wall"]), h


for _ in range(max(1, args.warmup)):        # graphs captured, sweep budgets settled
    run(True), run(False)
its = {True: [], False: []}
for _ in range(args.reps):
    for spec in (True, False):
        its[spec].append(run(spec)[0])
h = run(True)[1]
say()
say(f"iteration     final-time, memory 3, {args.iters} iterations a run, trials looked at {h['armijo_k']}, "
    f"cost {h['cost0']:.4e} -> {h['cost'][-1]:.4e}")
for spec in (True, False):
    a = np.array(its[spec])                 # (reps, iterations)
    med = np.median(a, axis=0)
    say(f"              {'speculative' if spec else 'sequential '}  per iteration (median over runs) "
        + "  ".join(f"{1e3 * m:8.2f}" for m in med) + f"   median of all {1e3 * np.median(a):8.2f} [{1e3 * a.min():.2f} .. "
        f"{1e3 * a.max():.2f}]")
say(f"              (a speculative iteration sweeps {K} members at once whatever it accepts; a sequential one sweeps the "
    f"trials it looks at one after the other)")

prob.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
