"""The set-ups that the tests of ``control_time=`` share between the CPU checks (test_control_intervals_oracle.py: the
reference loops descend, stay piecewise constant and decide their Armijo tests by margins >= 1e-8) and the GPU checks
(test_gpu_control_intervals.py: the device loops against these references).  Every reference is computed once per
process, in FEniCS DoF order, and is read-only.

Solid body: the set-up of test_gpu_lockstep.py (u0 = exp(-15((x+0.2)^2+(y-0.1)^2)), om = pi/40, eps = 0, c0 = 1, bounds
[0, 5], gam = 1e-4, s0 = 8, Nt = 6, dt = 1e-3 * 80/(N-1); all-time target = forward solve at c = 2, final-time target =
exp(-15((x+0.1)^2+(y-0.2)^2))), beta = 0.01, three iterations of up to six trials."""
import functools

import numpy as np

import control_intervals_oracle as cio

NT, OM, LO, HI, GAM, S0 = 6, np.pi / 40, 0.0, 5.0, 1e-4, 8.0
BETA, K_SB, ITERS_SB = 0.01, 6, 3
BETAS4 = [0.1, 0.03, 0.01, 0.001]
K_LS, ITERS_LS = 4, 2                     # the lockstep runs: test_gpu_lockstep.py's trial count and iterations
INTERVALS = {"stationary": (0, NT + 1), "0-3-4-7": (0, 3, 4, NT + 1), "identity": tuple(range(NT + 2))}
MARGIN_BAR = 1e-8                         # 1e5 x the solvers' 1e-13: the device cannot legitimately decide otherwise


def freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sb_case(N):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    om = SquareMesh(-1, 1, N - 1)
    asm = P1Assembler(om)
    n, dt = om.nodes, 1e-3 * 80 / (N - 1)
    tl = (NT + 1) * n
    sb = otraj.SolidBody(asm, om=OM)
    u0 = np.exp(-15 * ((om.x + 0.2) ** 2 + (om.y - 0.1) ** 2))[om.dof_to_vertex]
    uhat_T = np.exp(-15 * ((om.x + 0.1) ** 2 + (om.y - 0.2) ** 2))[om.dof_to_vertex]
    uhat_all = np.zeros(tl)
    uhat_all[:n] = u0
    otraj.solidbody_forward(sb, 2.0 * np.ones(tl), uhat_all, n, NT, dt)
    freeze(u0, uhat_T, uhat_all)
    return dict(mesh=om, sb=sb, n=n, dt=dt, tl=tl, u0=u0, finaltime=uhat_T, alltime=uhat_all, M=asm.mass())


@functools.lru_cache(maxsize=None)
def sb_oracle(N, optim, ivl, beta=BETA, K=K_SB, iters=ITERS_SB):
    """(u, c, hist) of the CPU loop with the intervals INTERVALS[ivl] (None: the oracle's own loop)"""
    cs = sb_case(N)
    starts = None if ivl is None else INTERVALS[ivl]
    u, _, c, h = cio.solidbody_pgd_loop(cs["sb"], cs["u0"], cs[optim], np.ones(cs["tl"]), beta, LO, HI, iters, cs["n"], NT,
                                        cs["dt"], starts, gam=GAM, s0=S0, max_armijo=K, optim=optim)
    freeze(u, c)
    return u, c, h


SB_CASES = [(N, optim, ivl) for N in (5, 21) for optim in ("alltime", "finaltime") for ivl in ("stationary", "0-3-4-7")]
LOCKSTEP_CASES = [(21, "alltime", "0-3-4-7"), (21, "finaltime", "stationary"), (46, "alltime", "stationary")]


# ---- snapshots: N = 21, the state observed at levels 2 and 6 on x < 0.25, first step length 1 (the snapshot weights
# carry no dt, so the gradient is larger than the all-time one and s0 = 8 is rejected throughout)
S0_SNAP = 1.0


@functools.lru_cache(maxsize=None)
def snap_oracle(Observations):
    cs = sb_case(21)
    x = cs["mesh"].x[cs["mesh"].dof_to_vertex]
    obs = Observations(NT, [2, NT], window=(x < 0.25).astype(np.float64))
    u, _, c, h = cio.solidbody_snapshots_pgd_loop(cs["sb"], cs["u0"], cs["alltime"], obs, np.ones(cs["tl"]), BETA, LO, HI,
                                                  ITERS_SB, cs["n"], NT, cs["dt"], INTERVALS["stationary"], gam=GAM,
                                                  s0=S0_SNAP, max_armijo=K_SB)
    freeze(u, c)
    return obs, u, c, h


# ---- source control: the reaction problem at the script's parameters, 11 x 11 nodes / 10 steps (test_gpu_reaction_source.py)
SRC = dict(nc=10, beta=0.1, lo=0.0, hi=1.0, eps=1e-4, iters=3)


@functools.lru_cache(maxsize=None)
def src_oracle(fields, wind, increment):
    """``fields`` / ``wind``: solvers.finaltime_exact_fields and solvers.finaltime_exact_wind() (the package's own)"""
    import reaction_source_oracle as rso
    pr = rso.script_problem(SRC["nc"], fields, wind)
    tl = (pr["Nt"] + 1) * pr["n"]
    res = cio.pgd_source_control(rso.script_reference(pr, SRC["eps"]), pr["u0"], pr["uhat_T"], np.zeros(tl), SRC["beta"],
                                 SRC["lo"], SRC["hi"], pr["n"], pr["Nt"], pr["dt"], (0, pr["Nt"] + 1), g=pr["F"]["f"],
                                 optim="finaltime", increment=increment, max_iters=SRC["iters"], tol=0.0, stop="cost",
                                 forward=rso.forward, adjoint=rso.adjoint)
    return pr, res


# ---- the three PDE systems: unit square 13 x 13, 8 steps (test_gpu_pdeco.py's mesh and step count)
SYS_NC, SYS_NT = 12, 8
MIMURA = (0.0, 1.0, -1.0)
SYSTEMS = {
    # name: (problem, dt, per_step, growth, intervals, iterations, options)
    "schnak-stationary-frozen": ("schnak", 1e-3, False, None, (0, SYS_NT + 1), 3, dict(max_iter_armijo=14)),
    "nonlinear-per-step-K2": ("nonlinear", 2e-3, True, None, (0, 5, SYS_NT + 1), 3, dict(optim="alltime")),
    "chtxs-stationary-growth": ("chtxs", 5e-4, True, MIMURA, (0, SYS_NT + 1), 2, dict(max_iter_armijo=8)),
}


@functools.lru_cache(maxsize=None)
def sys_case(name):
    """(asm, ic, targets, reference run); the targets are the problem's own sweep at a constant control (0.1 / 0.5 / 10)"""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    import chtxs_growth_oracle as go
    import per_step_oracle as po
    problem, dt, per_step, growth, starts, iters, opts = SYSTEMS[name]
    mesh = SquareMesh(0.0, 1.0, SYS_NC)
    asm = P1Assembler(mesh)
    n, Nt = mesh.nodes, SYS_NT
    tl = (Nt + 1) * n
    z = lambda x0: np.concatenate([x0, np.zeros(Nt * n)])
    ic = po.initial_conditions(problem, mesh)
    if problem == "nonlinear":
        ut, _ = otraj.solve_nonlinear_equation(np.full(tl, 0.5), z(ic[0]), None, asm, n, Nt, dt)
        targets = (ut.copy(),) if opts.get("optim") == "alltime" else (ut[Nt * n:].copy(),)
    elif problem == "schnak":
        ut, vt = otraj.solve_schnak_system(np.full(tl, 0.1), z(ic[0]), z(ic[1]), asm, n, Nt, dt)
        targets = (ut[Nt * n:].copy(), vt[Nt * n:].copy())
    else:
        ut, vt = go.solve_chtxs_system(np.full(tl, 10.0), z(ic[0]), z(ic[1]), asm, n, Nt, dt, growth=growth, per_step=True)
        targets = (ut.copy(), vt.copy())
    ref = cio.systems_pgd_loop(problem, asm, asm.mass(), ic, targets, Nt, dt, starts, iters, per_step=per_step,
                               growth=growth, **opts)
    freeze(*ic, *targets)
    return asm, ic, targets, ref
