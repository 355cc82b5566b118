#!/usr/bin/env python3
"""Fit the chemotaxis system with cell growth (Mimura-Tsujikawa) to two measured instants of one run on the MI355X backend.

The reference ships the cell density m and the chemoattractant f of one Mimura-Tsujikawa run at t = 14 and t = 30 on the
129 x 129 grid of [0,16]^2 (data/mimura_tsujikawa_t{14,30}_{m,f}.csv, about 320 KB each: not kept in this repository,
pass their directory with --data).  Its final-time script
(chemotaxis_mimura_FCT_PGD.py) can track one of them, its all-time script needs a whole trajectory; ``optim="snapshots"``
tracks both: levels 140 and 300 of a 300-step horizon with dt = 0.1,

    J = 1/2 sum_{n in {140, 300}} (||m_n - mhat_n||^2_M + ||f_n - fhat_n||^2_M) + beta/2 ||c||^2_Q.

Parameters of chemotaxis_mimura_FCT_PGD.py: delta = 32, Dm = 0.0625, Df = 1, chi = 8.5, eta = 0.5, growth m^2 (1 - m),
m0 = 1.5 + 0.1 (0.5 - rand) with seed 5, f0 = 1/32, 0 <= c <= 1.5, the state stepped with the control of its level.  The
files are in DoF order, as the script's comment says and the data itself shows.
The adjoint is loaded with the mass-weighted misfits (misfit="mass", the discrete adjoint of J).

``--reduced`` (the test suite's mode): every fourth node of the data (33 x 33, kept as
tests/golden/ref_data/mimura_tsujikawa_33x33_t{14,30}_{m,f}.csv in the DoF order of the 33 x 33 mesh: the same format and
the same read path as the full-size files), 6 steps, levels 3 and 6.

usage: python examples/chemotaxis_mimura_snapshots_pdeco.py (--data DIR | --reduced) [--iters 3] [--misfit mass|nodal]"""
import argparse
import os
import time

import numpy as np

from _common import ROOT, hp, solvers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--reduced", action="store_true")
ap.add_argument("--data", default=None, help="directory with the reference's mimura_tsujikawa_t{14,30}_{m,f}.csv (full size)")
ap.add_argument("--misfit", choices=["mass", "nodal"], default="mass")
args = ap.parse_args()
if not args.reduced and args.data is None:
    ap.error("the full-size run needs --data DIR (the reference's data directory); --reduced runs on the committed fixtures")
data_dir = args.data if args.data is not None else os.path.join(ROOT, "tests", "golden", "ref_data")

FULL = 129
N = 33 if args.reduced else FULL
Nt, levels = (6, [3, 6]) if args.reduced else (300, [140, 300])
dt, growth = 0.1, (0.0, 1.0, -1.0)
par = [32.0, 0.0625, 1.0, 8.5, 0.5]                 # delta, Dm, Df, chi, eta

V = hp.SquareMeshP1(0.0, 16.0, N - 1)
n = V.nodes


def snapshot(name):
    """a snapshot of the run: one line of comma-separated values in the DoF order of this mesh"""
    prefix = "mimura_tsujikawa_33x33_" if args.reduced else "mimura_tsujikawa_"
    a = np.genfromtxt(os.path.join(data_dir, f"{prefix}{name}.csv"), delimiter=",").ravel()
    if a.size != n:
        raise SystemExit(f"{name}: {a.size} values, expected {n}")
    return a


mhat, fhat = np.full((Nt + 1) * n, np.nan), np.full((Nt + 1) * n, np.nan)       # only the observed levels are read
for lv, t in zip(levels, (14, 30)):
    mhat[lv * n:(lv + 1) * n], fhat[lv * n:(lv + 1) * n] = snapshot(f"t{t}_m"), snapshot(f"t{t}_f")

np.random.seed(5)
m0 = hp.reorder_vector_to_dof(1.5 + 0.1 * (0.5 - np.random.rand(N, N)).reshape(n), 1, n, V.vertex_to_dof)
f0 = np.full(n, 1 / 32)

obs = solvers.Observations(Nt, levels)
print(f"Mimura-Tsujikawa snapshots: {N} x {N} nodes on [0,16]^2, {Nt} steps of dt = {dt}, levels {levels}, misfit = {args.misfit}")
t0 = time.perf_counter()
with hp.SystemPDECO("chtxs", V, Nt, dt, optim="snapshots", obs=obs, misfit=args.misfit, growth=growth, control_per_step=True,
                    par=par, c_lower=0.0, c_upper=1.5, max_iter_GD=args.iters, tol=0.0) as prob:
    res = prob.run((m0, f0), (mhat, fhat), speculative=True)
el = time.perf_counter() - t0
print(f"{res['it']} PGD iterations in {el:.2f} s, restored = {res['restored']}")
for k, J in enumerate(res["cost"]):
    trials = res["armijo_its"][k - 1] if k else "-"
    print(f"  it {k:2d}  cost {J:.8e}   Armijo trials {trials}")
print(f"control: min {res['c'].min():.4f}  mean {res['c'].mean():.4f}  max {res['c'].max():.4f}")
