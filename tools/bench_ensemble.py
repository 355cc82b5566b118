#!/usr/bin/env python3
"""Measurements of the ensemble drift control at config C2's size (81 x 81 P1 nodes, n = 6561, 250 steps of 1e-3) for
S = 4, 16, 64 scenarios; writes profiles/ensemble.txt.  Per S, medians of --reps timed repetitions after --warmup untimed
ones, every timed region closed by a device synchronise, on an otherwise idle device:

  direction   one femfct_ensemble_drift_gradient_rhs launch + one batched ChebSI, against what the library offered
              before for the same result: S x descent_direction into S buffers + q_combine (17 fields a call)
  costs       ensemble_costs against obs_cost of S members + l2_norm_sq_Q of the control and of its distance
  iteration   --iters ensemble iterations against S single-scenario lbfgs_solidbody runs of --iters iterations, one after
              the other (sequential search in both, memory 0)
  bandwidth   the rhs kernel alone: (2S + 2) trajectories of compulsory traffic over its time

usage: python tools/bench_ensemble.py [--out profiles/ensemble.txt] [--sizes 4 16 64] [--reps 7] [--warmup 2] [--iters 2]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble.txt"))
ap.add_argument("--sizes", type=int, nargs="+", default=[4, 16, 64])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--cells", type=int, default=80)
ap.add_argument("--steps", type=int, default=250)
args = ap.parse_args()

nc, Nt, dt = args.cells, args.steps, 1e-3
beta, lo, hi = 1e-3, 0.0, 5.0
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


def median_time(fn, inner=1):
    """per call: a repetition is ``inner`` calls back to back and one synchronise (a launch of ~0.1 ms alone would time
    the host clock and the enqueue)"""
    for _ in range(args.warmup):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t) / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


say(f"# ensemble drift control, n = {n}, {Nt} steps, build {hp._lib.lib.femfct_build_id().decode()}")
say(f"# medians of {args.reps} repetitions after {args.warmup} warm-ups (min .. max in brackets), milliseconds")
for S in args.sizes:
    ang = 2 * np.pi * np.arange(S) / S
    u0 = np.stack([np.exp(-15 * ((x - 0.25 * np.cos(a)) ** 2 + (y - 0.25 * np.sin(a)) ** 2)) for a in ang])
    w = (1.0 + np.arange(S) % 3) / np.sum(1.0 + np.arange(S) % 3)
    c = ctx.array(np.ones(tl) + 0.1 * np.tile(x, levels))
    cref = ctx.array(np.ones(tl))
    u, p, uh = ctx.zeros(S * tl), ctx.zeros(S * tl), ctx.zeros(S * tl)
    for s in range(S):
        row = ctx.array(u0[s])
        u.copy_from(row, n, dst_off=s * tl)
        uh.copy_from(row, n, dst_off=s * tl)
        row.free()
    two = ctx.array(np.full(tl, 2.0))
    prob.forward(two, uh, batch=S, c_shared=True)           # targets: the states under the constant control 2
    prob.forward(c, u, batch=S, c_shared=True)
    obs = solvers.Observations.finaltime(Nt)
    theta, cost_w, window = prob.obs_device(obs)
    ctx.solidbody_adjoint_obs(prob.Arot, c, u, uh, theta, obs.tau, window, p, Nt, dt, prob.eps, prob.rot_scale, prob.drift,
                              S, True)
    say()
    say(f"S = {S}   (sweep kernels: regime {ctx.kernel_regime(S)} at batch S, {ctx.kernel_regime(1)} at batch 1)")

    # -- direction
    rhs, d = ctx.empty(tl), ctx.empty(tl)
    new_dir = lambda: (ctx.ensemble_drift_gradient_rhs(c, u, p, w, beta, rhs, levels, prob.drift),
                       ctx.chebsi(rhs, d, 20, 0.5, 2.0, batch=levels))
    ds = [ctx.empty(tl) for _ in range(S)]
    acc = [ctx.empty(tl), ctx.empty(tl)]

    def old_dir():
        # d = ChebSI(-(beta M c + sum pi_s G_s)) = sum_s pi_s ChebSI(-(beta M c + G_s)) for weights of sum 1 (ChebSI is linear)
        for s in range(S):
            prob.descent_direction(c, u.ptr + 8 * s * tl, p.ptr + 8 * s * tl, beta, ds[s], scratch=rhs)
        k, cur = 0, None
        while k < S:
            take = ds[k:k + (17 if cur is None else 16)]
            coef = list(w[k:k + len(take)])
            fields = take if cur is None else [acc[cur]] + take
            nxt = 0 if cur is None else 1 - cur
            ctx.q_combine(fields, coef if cur is None else [1.0] + coef, tl, acc[nxt])
            cur, k = nxt, k + len(take)

    t_new, t_old = median_time(new_dir, 10), median_time(old_dir, 2)
    say(f"  direction   ensemble {1e3 * t_new[0]:9.3f} [{1e3 * t_new[1]:.3f} .. {1e3 * t_new[2]:.3f}]   "
        f"S x descent_direction + q_combine {1e3 * t_old[0]:9.3f} [{1e3 * t_old[1]:.3f} .. {1e3 * t_old[2]:.3f}]   "
        f"ratio {t_old[0] / t_new[0]:.2f}")

    # -- the rhs kernel alone
    t_rhs = median_time(lambda: ctx.ensemble_drift_gradient_rhs(c, u, p, w, beta, rhs, levels, prob.drift), 20)
    t_one = median_time(lambda: ctx.drift_gradient_rhs(c, u, p, beta, rhs, levels, prob.drift), 20)
    byts, byts1 = (2 * S + 2) * tl * 8, 4 * tl * 8
    say(f"  rhs kernel  {1e3 * t_rhs[0]:9.3f} [{1e3 * t_rhs[1]:.3f} .. {1e3 * t_rhs[2]:.3f}]   {byts / 1e6:.1f} MB compulsory, "
        f"{byts / t_rhs[0] / 1e12:.3f} TB/s = {byts / t_rhs[0] / 8e12:.3f} of 8 TB/s   (20 launches back to back per repetition; "
        f"drift_gradient_rhs alone: {1e3 * t_one[0]:.3f} ms, {byts1 / t_one[0] / 1e12:.3f} TB/s)")

    # -- costs
    t_cn = median_time(lambda: ctx.ensemble_costs(u, uh, cost_w, c, w, beta, Nt, dt, cref=cref))
    t_co = median_time(lambda: (ctx.obs_cost(u, uh, cost_w, Nt, batch=S), ctx.l2_norm_sq_Q(c, None, Nt, dt),
                                ctx.l2_norm_sq_Q(c, cref, Nt, dt)))
    say(f"  costs       ensemble {1e3 * t_cn[0]:9.3f} [{1e3 * t_cn[1]:.3f} .. {1e3 * t_cn[2]:.3f}]   "
        f"obs_cost + 2 x l2_norm_sq_Q {1e3 * t_co[0]:9.3f} [{1e3 * t_co[1]:.3f} .. {1e3 * t_co[2]:.3f}]   "
        f"ratio {t_co[0] / t_cn[0]:.2f}")
    for a in [c, cref, u, p, two, rhs, d] + ds + acc:
        a.free()

    # -- iteration
    uhat_T = uh.download().reshape(S, tl)[:, Nt * n:].copy()
    uh.free()
    ens = solvers.Ensemble(u0, uhat_T, w)
    c0 = np.ones(tl)
    run_e = lambda: solvers.ensemble_solidbody(prob, ens, c0, beta, lo, hi, args.iters, memory=0, s0=64.0)
    run_s = lambda: [solvers.lbfgs_solidbody(prob, u0[s], uhat_T[s], c0, beta, lo, hi, args.iters, memory=0, s0=64.0,
                                             speculative=False) for s in range(S)]
    run_e(), run_s()            # warm-up: graphs captured, sweep budgets settled
    t = time.perf_counter()
    he = run_e()[3]
    t_e = time.perf_counter() - t
    t = time.perf_counter()
    hs = run_s()
    t_s = time.perf_counter() - t
    sw_e, sw_s = he["sweeps"][-1], sum(h[3]["sweeps"][-1] for h in hs)
    say(f"  iteration   {args.iters} ensemble iterations {t_e:8.3f} s ({sw_e} sweeps of {S} members, "
        f"{sw_e * S * Nt / t_e / 1e3:.0f} k member-steps/s)   {S} x lbfgs_solidbody {t_s:8.3f} s ({sw_s} sweeps of 1, "
        f"{sw_s * Nt / t_s / 1e3:.0f} k steps/s)   time per member-sweep: ratio {(t_s / sw_s) / (t_e / (sw_e * S)):.2f}")

prob.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
