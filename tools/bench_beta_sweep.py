#!/usr/bin/env python3
"""Config C5's regularisation sweep (81 x 81, 100 steps of dt = 1e-3, no rotation, eight beta = 10^(-k/2), all-time misfit,
max_armijo = 8, three iterations) run two ways on one GPU:

  (a) sequential   eight pgd_solidbody_alltime runs in turn (speculative), what examples/c5_beta_sweep.py does
  (b) lockstep     one pgd_solidbody_lockstep call

Each run is on a fresh context after one untimed warm-up iteration (graph capture); the two alternate --reps times.
Iteration times come from hist["wall"] (every entry follows a read-back of the iteration's costs: synchronised).  Then,
with the phases of one run of each bracketed by device synchronisations, where the time goes; and femfct_member_costs
against the path it replaces (femfct_cost_functional + femfct_l2_norm_sq_Q on replicated targets and controls) on the
same 64 members, median of 7 synchronised calls.

usage: python tools/bench_beta_sweep.py [--reps 3] > profiles/r11_beta_sweep.txt"""
import argparse
import importlib
import os
import sys
import time
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hp = importlib.import_module("fem-fct-pdeco_amd")
solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--iters", type=int, default=3)
args = ap.parse_args()

a1, a2, nc, dt, K = -1.0, 1.0, 80, 1e-3, 8
mesh = hp.SquareMeshP1(a1, a2, nc)
n, Nt = mesh.nodes, args.steps
tl = (Nt + 1) * n
betas = [10.0 ** (-k / 2) for k in range(8)]
P = len(betas)
REGIMES = {getattr(hp._lib, k): k[7:] for k in dir(hp._lib) if k.startswith("REGIME_")}
X = np.linspace(a1, a2, nc + 1)
XX, YY = np.meshgrid(X, X)
u0 = np.exp(-20 * ((XX + 2 / 3) ** 2 + 5 * (YY + 5 / 6) ** 2)).reshape(-1)      # advection_solidbody_FCT_PDECO_alltime.py:93-96
c0 = np.ones(tl)


def new_prob():
    return solvers.SolidBodyDrift(mesh, Nt, dt, eps=0.0, drift=(1.0, 1.0), rot_scale=0.0, order=hp.ORDER_VERTEX)


prob = new_prob()
uhat = np.zeros(tl)
uhat[:n] = u0
uhat = prob.solve_state(2.0 * np.ones(tl), uhat)            # target trajectory at the true control c = 2
prob.close()


def run_sequential(prob, iters, which=betas):
    return [solvers.pgd_solidbody_alltime(prob, u0, uhat, c0, b, 0.0, 5.0, iters, max_armijo=K) for b in which]


def run_lockstep(prob, iters):
    return solvers.pgd_solidbody_lockstep(prob, u0, uhat, c0, betas, 0.0, 5.0, iters, max_armijo=K, optim="alltime")


def timed(kind):
    """(whole-run wall seconds, seconds inside the iterations from hist["wall"], results) on a fresh, warmed context"""
    prob = new_prob()
    try:
        if kind == "a":
            run_sequential(prob, 1, betas[:1])
        else:
            run_lockstep(prob, 1)
        prob.ctx.synchronize()
        t0 = time.perf_counter()
        res = run_sequential(prob, args.iters) if kind == "a" else run_lockstep(prob, args.iters)
        prob.ctx.synchronize()
        wall = time.perf_counter() - t0
        if kind == "a":
            inner = sum(r[3]["wall"][-1] - r[3]["wall0"] for r in res)
        else:
            inner = max(r[3]["wall"][-1] for r in res) - res[0][3]["wall0"]
        return wall, inner, res, prob.ctx.kernel_regime(1), prob.ctx.kernel_regime(K)
    finally:
        prob.close()


print(f"# build {hp._lib.lib.femfct_build_id().decode()}: config C5, {nc + 1}^2 nodes, {Nt} steps, {P} beta, max_armijo = {K}, "
      f"{args.iters} iterations, all-time; fresh context + one warm-up iteration per run; {args.reps} alternating repetitions")
print("# rep  (a) sequential: run_ms  iterations_ms   (b) lockstep: run_ms  iterations_ms   a/b (run)  a/b (iterations)")
rows = []
for rep in range(args.reps):
    wa, ia, ra, reg1, regK = timed("a")
    wb, ib, rb, _, _ = timed("b")
    rows.append((wa, ia, wb, ib))
    print(f"  {rep}    {wa * 1e3:10.2f}  {ia * 1e3:10.2f}     {wb * 1e3:10.2f}  {ib * 1e3:10.2f}     {wa / wb:6.2f}  {ia / ib:6.2f}")
med = np.median(np.array(rows), axis=0)
print(f"# median  {med[0] * 1e3:10.2f}  {med[1] * 1e3:10.2f}     {med[2] * 1e3:10.2f}  {med[3] * 1e3:10.2f}     "
      f"{med[0] / med[2]:6.2f}  {med[1] / med[3]:6.2f}")
print(f"# (a) launches: batch 1 (adjoint, first state; regime {REGIMES[reg1]}) and batch {K} (trials; regime {REGIMES[regK]}), "
      f"{P} runs x {args.iters} iterations")
rec = rb.record
print(f"# (b) launches: problems per iteration {rec['problems']} (regimes {[REGIMES[r] for r in rec['regime_problems']]}), "
      f"trial members {rec['trials']} (regimes {[REGIMES[r] for r in rec['regime_trials']]})")
ja, jb = np.array([r[3]["cost"] for r in ra]), np.array([r[3]["cost"] for r in rb])
print(f"# same iterates: armijo_k equal {[r[3]['armijo_k'] for r in ra] == [r[3]['armijo_k'] for r in rb]}, "
      f"max relative cost difference {np.max(np.abs(ja - jb) / np.abs(ja)):.2e}, "
      f"max relative l2 difference of c {max(np.linalg.norm(x[2] - y[2]) / np.linalg.norm(x[2]) for x, y in zip(ra, rb)):.2e}")
for b, x, y in zip(betas, ja, jb):
    print(f"#   beta = {b:9.3e}   J (a) = {x[-1]:.10e}   J (b) = {y[-1]:.10e}")

# ---- phases, bracketed by synchronisations (the brackets cost overlap: the sums exceed the unbracketed runs)
acc, cnt = defaultdict(float), defaultdict(int)


def wrap(obj, name, ctx, label):
    f = getattr(obj, name)

    def g(*a, **k):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = f(*a, **k)
        ctx.synchronize()
        lab = label(a, k) if callable(label) else label
        acc[lab] += time.perf_counter() - t0
        cnt[lab] += 1
        return r
    setattr(obj, name, g)


def phases(kind):
    acc.clear()
    cnt.clear()
    prob = new_prob()
    try:
        if kind == "a":
            run_sequential(prob, 1, betas[:1])
        else:
            run_lockstep(prob, 1)
        ctx = prob.ctx
        wrap(prob, "adjoint", ctx, "adjoint")
        first = 1 if kind == "a" else P          # batch of the first state sweep; the other forward sweeps are trials
        wrap(prob, "forward", ctx, lambda a, k: "state" if k.get("batch") == first else "trials")
        if kind == "a":
            wrap(prob, "descent_direction", ctx, "direction")
            wrap(prob, "cost", ctx, "costs")
            wrap(ctx, "l2_norm_sq_Q", ctx, "costs")
            wrap(ctx, "project_control", ctx, "controls")
        else:
            wrap(ctx, "drift_gradient_rhs", ctx, "direction")
            wrap(ctx, "chebsi", ctx, "direction")
            wrap(ctx, "member_costs", ctx, "costs")
            wrap(ctx, "trial_controls", ctx, "controls")
        ctx.synchronize()
        t0 = time.perf_counter()
        run_sequential(prob, args.iters) if kind == "a" else run_lockstep(prob, args.iters)
        ctx.synchronize()
        el = time.perf_counter() - t0
        out = {k: (acc[k], cnt[k]) for k in acc}
        out["other (copies, set-up, downloads)"] = (el - sum(acc.values()), 0)
        return el, out
    finally:
        prob.close()


print("# phases of one run, every phase between device synchronisations; ms (calls)")
print("# phase                               (a) sequential        (b) lockstep")
(ea, pa), (eb, pb) = phases("a"), phases("b")
for k in ("adjoint", "direction", "state", "trials", "costs", "controls", "other (copies, set-up, downloads)"):
    xa, ca = pa.get(k, (0.0, 0))
    xb, cb = pb.get(k, (0.0, 0))
    print(f"  {k:34s} {xa * 1e3:9.2f} ({ca:3d})     {xb * 1e3:9.2f} ({cb:3d})")
print(f"  {'whole run':34s} {ea * 1e3:9.2f}           {eb * 1e3:9.2f}")

# ---- femfct_member_costs against femfct_cost_functional + femfct_l2_norm_sq_Q on the same 64 members
prob = new_prob()
ctx = prob.ctx
rng = np.random.default_rng(11)
B = P * K
uB, cB = ctx.array(rng.random(B * tl)), ctx.array(5.0 * rng.random(B * tl))
c, uh = ctx.array(5.0 * rng.random(P * tl)), ctx.array(uhat)
uhB, ckB = ctx.empty(B * tl), ctx.empty(B * tl)            # what the old path needs: a target and a control per member
for m in range(B):
    uhB.copy_from(uh, tl, dst_off=m * tl)
    ckB.copy_from(c, tl, dst_off=m * tl, src_off=(m // K) * tl)
beta1 = [betas[0]] * P                                     # (the old path takes one beta per call)


def old():
    return (ctx.cost_functional(uB, uhB, cB, Nt, dt, beta1[0], "alltime", batch=B), ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=B))


def new():
    return ctx.member_costs(uB, uh, cB, beta1, P, K, Nt, dt, "alltime", cref=c)


def median7(fn):
    fn()
    t = []
    for _ in range(7):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()                      # both paths return after reading their scalars back: synchronised
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


t_old, t_new, t_old2 = median7(old), median7(new), median7(old)
(Jo, do), (Jn, dn) = old(), new()
by_old, by_new = 5 * B * tl * 8, (2 * B + 1 + P) * tl * 8
print(f"# costs of {B} members ({P} problems x {K} trials), {Nt + 1} levels x {n} nodes, median of 7 synchronised calls")
print(f"  cost_functional + l2_norm_sq_Q (replicated target, control): {t_old * 1e3:8.3f} ms, again after: {t_old2 * 1e3:8.3f} ms; "
      f"compulsory {by_old / 1e6:.1f} MB ({by_old / min(t_old, t_old2) / 1e9:.0f} GB/s)")
print(f"  member_costs (one fused pass):                               {t_new * 1e3:8.3f} ms; "
      f"compulsory {by_new / 1e6:.1f} MB ({by_new / t_new / 1e9:.0f} GB/s); old/new = {min(t_old, t_old2) / t_new:.2f}")
print(f"  same bits: J {np.array_equal(Jo, Jn)}, dist {np.array_equal(do, dn)}")
prob.close()
