#!/usr/bin/env python3
"""The control budget at config C2's size (81 x 81 nodes, 251 levels, one trajectory of 13.2 MB, K = 10 trials):

  budget_trials, every trial over the budget     the whole call: the writing pass, the search rounds (one launch and one
                                                 read-back of 19 K doubles each), the writing pass again; rounds used
  budget_trials, a budget nothing reaches        the writing pass alone (femfct_prox_trials' values, norms, max |x|)
  per search round                               (the first minus twice the second) / rounds
  prox_trials                                    on the same inputs: what the loops launch without a budget
  a prox_solidbody iteration                     with and without a budget, from the loops' own wall-clock history

Times are the median over --reps of --calls back-to-back calls between two device synchronisations, divided by the
number of calls, after a warm-up (budget_trials synchronises itself: its times include the read-backs).  The whole
measurement is repeated --rounds times.  --no-budget leaves out everything that needs femfct_budget_trials, so that the
same tool times a build without it (the parent of the change) for the comparison.

usage: python tools/bench_budget.py [--reps 7] [--calls 5] [--rounds 3] [--iters 3] [--no-budget] > profiles/control_budgets.txt"""
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
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--no-budget", action="store_true")
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
alpha, lo, hi = 1e-3, -0.1, 0.5
mesh = hp.SquareMeshP1(-1.0, 1.0, nc)
prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=np.pi / 40, order=hp.ORDER_VERTEX)
ctx, n, tl = prob.ctx, prob.n, prob.tlen
MB = 8 * tl / 1e6
print(f"# build {hp._lib.lib.femfct_build_id().decode()}: n = {n}, {Nt + 1} levels, trajectory {MB:.2f} MB, K = {K}; median of "
      f"{args.reps} x ({args.calls} calls between two synchronisations) / {args.calls}, {args.rounds} rounds"
      f"{'; without femfct_budget_trials' if args.no_budget else ''}")
rng = np.random.default_rng(17)
# |c| small, |d| over four decades: the norm of trial t falls with t, and a budget of 1e-3 of trial K-1's keeps all K over it
c = ctx.array(rng.uniform(-0.02, 0.02, tl))
d = ctx.array(rng.standard_normal(tl) * 10.0 ** rng.uniform(-3, 1, tl))
cB = ctx.empty(K * tl)
ctx.prox_trials(c, d, 1.0, K, alpha, lo, hi, tl, cB)
norms = ctx.l1_norm_Q(cB, Nt, dt, batch=K)
cases = [("prox_trials", lambda: ctx.prox_trials(c, d, 1.0, K, alpha, lo, hi, tl, cB))]
if not args.no_budget:
    B = 0.3 * float(norms.min())
    lam, l1, rounds = ctx.budget_trials(c, d, 1.0, K, alpha, B, lo, hi, Nt, dt, cB)
    assert np.all(lam > 0), "every trial was meant to be over the budget"
    print(f"# budget {B:.6e} = 0.3 of the smallest trial norm: rounds per trial {rounds.tolist()}, "
          f"max |l1 / B - 1| = {np.abs(l1 / B - 1).max():.1e}")
    cases += [("budget_trials, all over budget", lambda: ctx.budget_trials(c, d, 1.0, K, alpha, B, lo, hi, Nt, dt, cB)),
              ("budget_trials, budget 1e300", lambda: ctx.budget_trials(c, d, 1.0, K, alpha, 1e300, lo, hi, Nt, dt, cB))]
rows = {name: [] for name, _ in cases}
for _ in range(args.rounds):
    for name, fn in cases:
        rows[name].append(timed(ctx, fn))
print("\n## microseconds per call (median of the rounds; every round)")
for name, _ in cases:
    print(f"{name:34s} {float(np.median(rows[name])):10.1f}   ({'  '.join(f'{v:9.1f}' for v in rows[name])})")
if not args.no_budget:
    tb, ts, tp = (float(np.median(rows[k])) for k in ("budget_trials, all over budget", "budget_trials, budget 1e300", "prox_trials"))
    r = int(rounds.max())
    print(f"\nsearch rounds of the call                     {r}")
    print(f"per search round, (all over - 2 x 1e300) / {r:<3d}  {(tb - 2 * ts) / r:.1f} us   "
          f"(nominal traffic K x (c + d) = {2 * K * MB:.0f} MB, distinct {2 * MB:.0f} MB)")
    print(f"budget_trials (all over budget) / prox_trials {tb / tp:.1f}")
    print(f"budget_trials (budget 1e300) / prox_trials    {ts / tp:.1f}")

# one iteration of prox_solidbody: a Gaussian bump carried a quarter turn, final-time tracking, c0 = 0
x, y = mesh.coordinates()        # (vertex order: the problem's node order here)
u0 = np.exp(-((x - 0.4) ** 2 + y ** 2) / 0.02)
uhat = np.exp(-(x ** 2 + (y - 0.4) ** 2) / 0.02)


def iteration_ms(**kw):
    out = []
    for _ in range(args.rounds):
        h = solvers.prox_solidbody(prob, u0, uhat, np.zeros(tl), 1e-4, 0.0, lo, hi, args.iters, s0=64.0, max_armijo=K, **kw)[3]
        w = np.diff([h["wall0"]] + h["wall"])
        out.append(1e3 * float(np.median(w[1:] if len(w) > 1 else w)))
    return out, h


print(f"\n## a prox_solidbody iteration (alpha = 0, K = {K}, final-time tracking), milliseconds: median over iterations 2.."
      f"{args.iters} of every round")
free, hf = iteration_ms()
print(f"{'no budget':34s} {float(np.median(free)):10.1f}   ({'  '.join(f'{v:9.1f}' for v in free)})   armijo_k {hf['armijo_k']}")
if not args.no_budget and hf["l1"]:
    Bl = 0.3 * hf["l1"][-1]
    with_b, hb = iteration_ms(budget=Bl)
    print(f"{'budget = 0.3 of its final norm':34s} {float(np.median(with_b)):10.1f}   ({'  '.join(f'{v:9.1f}' for v in with_b)})   "
          f"armijo_k {hb['armijo_k']}, rounds {hb['projection_rounds']}, multiplier {['%.3g' % m for m in hb['multiplier']]}")
    print(f"with / without                                {np.median(with_b) / np.median(free):.3f}   "
          f"(the two runs take different steps: the iterations are not the same work)")
prob.close()
