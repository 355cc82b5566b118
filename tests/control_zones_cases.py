"""The set-ups that the tests of ``control_space=`` share between the CPU checks (test_control_zones_oracle.py: the
reference loops descend, stay zone-constant and decide their Armijo tests by margins >= 1e-8) and the GPU checks
(test_gpu_control_zones.py: the device loops against these references).  Every reference is computed once per process, in
FEniCS DoF order, and is read-only.

The solid-body set-ups are those of control_intervals_cases.sb_case (N = 5 and 21, Nt = 6, beta = 0.01, bounds [0, 5],
s0 = 8, up to six trials, three iterations) with two layouts of zones:

    quadrants   boundary nodes -1, interior nodes (x > 0.1) + 2 (y > -0.3): unequal zones, 2/1/4/2 nodes at N = 5 and
                60/54/130/117 at N = 21
    mod3        label_i = i mod 3 in DoF order: scattered gathers, no inactive node

with the free time dependence and with the intervals (0, 3, 4, 7).  One more case makes the box active: N = 21, quadrants,
all-time, c_lower = 0.62 (the control reaches the bound in the third iteration)."""
import functools

import numpy as np

import control_intervals_cases as cc
import control_zones_oracle as czo

NT, LO, HI, GAM, S0, BETA, K_SB, ITERS_SB = cc.NT, cc.LO, cc.HI, cc.GAM, cc.S0, cc.BETA, cc.K_SB, cc.ITERS_SB
MARGIN_BAR = cc.MARGIN_BAR
IVL = "0-3-4-7"
LO_ACTIVE = 0.62
freeze = cc.freeze


@functools.lru_cache(maxsize=None)
def layout(N, name):
    """(labels in DoF order, m)"""
    om = cc.sb_case(N)["mesh"]
    x, y = om.x[om.dof_to_vertex], om.y[om.dof_to_vertex]
    if name == "quadrants":
        edge = (np.abs(np.abs(x) - 1.0) < 1e-12) | (np.abs(np.abs(y) - 1.0) < 1e-12)
        lab = np.where(edge, -1, (x > 0.1).astype(np.int64) + 2 * (y > -0.3))
    elif name == "mod3":
        lab = np.arange(om.nodes) % 3
    elif name == "one":
        lab = np.zeros(om.nodes, dtype=np.int64)
    elif name == "each":
        lab = np.arange(om.nodes)
    elif name == "lone":
        lab = np.full(om.nodes, -1)
        lab[om.nodes // 2 + 1] = 0
    else:
        raise KeyError(name)
    lab = lab.astype(np.int32)
    freeze(lab)
    return lab, int(lab.max()) + 1


def starts_of(ivl):
    return None if ivl is None else cc.INTERVALS[ivl]


@functools.lru_cache(maxsize=None)
def sb_oracle(N, name, optim, ivl, c_lower=LO, cheb=False):
    """(u, c, hist) of the CPU loop with the zones of ``layout(N, name)`` and the intervals INTERVALS[ivl] (None: free in
    time); ``cheb``: the direction formed as P(ChebSI(rhs))"""
    cs = cc.sb_case(N)
    lab, m = layout(N, name)
    u, _, c, h = czo.solidbody_pgd_loop(cs["sb"], cs["u0"], cs[optim], np.ones(cs["tl"]), BETA, c_lower, HI, ITERS_SB,
                                        cs["n"], NT, cs["dt"], lab, m, starts_of(ivl), cheb=cheb, gam=GAM, s0=S0,
                                        max_armijo=K_SB, optim=optim)
    freeze(u, c)
    return u, c, h


SB_CASES = [(N, name, optim, ivl) for N in (5, 21) for name in ("quadrants", "mod3") for optim in ("alltime", "finaltime")
            for ivl in (None, IVL)]
ACTIVE_CASE = (21, "quadrants", "alltime", None)


@functools.lru_cache(maxsize=None)
def snap_oracle(Observations):
    """control_intervals_cases.snap_oracle's window case (levels 2 and 6 on x < 0.25, s0 = 1) on quadrants, free in time"""
    cs = cc.sb_case(21)
    lab, m = layout(21, "quadrants")
    x = cs["mesh"].x[cs["mesh"].dof_to_vertex]
    obs = Observations(NT, [2, NT], window=(x < 0.25).astype(np.float64))
    u, _, c, h = czo.solidbody_snapshots_pgd_loop(cs["sb"], cs["u0"], cs["alltime"], obs, np.ones(cs["tl"]), BETA, LO, HI,
                                                  ITERS_SB, cs["n"], NT, cs["dt"], lab, m, gam=GAM, s0=cc.S0_SNAP,
                                                  max_armijo=K_SB)
    freeze(u, c)
    return obs, u, c, h


LBFGS_SB = dict(N=21, name="quadrants", optim="alltime", iters=3, memory=5)


@functools.lru_cache(maxsize=None)
def lbfgs_sb_oracle():
    L = LBFGS_SB
    cs = cc.sb_case(L["N"])
    lab, m = layout(L["N"], L["name"])
    u, _, c, h = czo.lbfgs_solidbody(cs["sb"], cs["u0"], cs[L["optim"]], np.ones(cs["tl"]), BETA, LO, HI, L["iters"], cs["n"],
                                     NT, cs["dt"], lab, m, memory=L["memory"], gam=GAM, s0=S0, max_armijo=K_SB,
                                     optim=L["optim"])
    freeze(u, c)
    return u, c, h


# ---- source control: control_intervals_cases' reaction problem (11 x 11 nodes, 10 steps) with a 2 x 2 layout of blocks.
# The upper bound is 4, not that set-up's 1: with four amplitudes per level the first step puts every zone on the bound 1,
# every later trial equals the iterate and its Armijo margin is exactly 0, a tie no implementation can be held to.  At 4
# two zones reach the bound and two stay inside, the third linear search rejects a trial, and every margin is >= 4e-3.
SRC = dict(cc.SRC, hi=4.0)


def blocks_labels(mesh, bx, by, margin=0):
    """bx x by rectangles over the nodes inside ``margin`` node rows, -1 outside, in the DoF order of the oracle's mesh"""
    N = mesh.N
    inner = N - 2 * margin
    iy, ix = np.divmod(np.arange(mesh.nodes), N)
    inside = (ix >= margin) & (ix < N - margin) & (iy >= margin) & (iy < N - margin)
    lab = np.where(inside, ((iy - margin) * by // inner) * bx + (ix - margin) * bx // inner, -1)
    return lab[mesh.dof_to_vertex].astype(np.int32)


@functools.lru_cache(maxsize=None)
def src_problem(fields, wind):
    import reaction_source_oracle as rso
    pr = rso.script_problem(SRC["nc"], fields, wind)
    lab = blocks_labels(pr["mesh"], 2, 2)
    freeze(lab)
    return pr, rso.script_reference(pr, SRC["eps"]), lab


@functools.lru_cache(maxsize=None)
def src_oracle(fields, wind, increment):
    import reaction_source_oracle as rso
    pr, rs, lab = src_problem(fields, wind)
    tl = (pr["Nt"] + 1) * pr["n"]
    proj = czo.source_projection(rs.cm.M, lab, 4, None, pr["Nt"], pr["n"])
    res = czo.pgd_source_control(rs, pr["u0"], pr["uhat_T"], np.zeros(tl), SRC["beta"], SRC["lo"], SRC["hi"], pr["n"],
                                 pr["Nt"], pr["dt"], proj, g=pr["F"]["f"], optim="finaltime", increment=increment,
                                 max_iters=SRC["iters"], tol=0.0, stop="cost", forward=rso.forward, adjoint=rso.adjoint)
    return pr, lab, res


@functools.lru_cache(maxsize=None)
def lbfgs_src_oracle(fields, wind):
    import reaction_source_oracle as rso
    pr, rs, lab = src_problem(fields, wind)
    tl = (pr["Nt"] + 1) * pr["n"]
    proj = czo.source_projection(rs.cm.M, lab, 4, None, pr["Nt"], pr["n"])
    res = czo.lbfgs_source_control(rs, pr["u0"], pr["uhat_T"], np.zeros(tl), SRC["beta"], SRC["lo"], SRC["hi"], SRC["iters"],
                                   pr["n"], pr["Nt"], pr["dt"], proj, g=pr["F"]["f"], optim="finaltime", memory=5,
                                   forward=rso.forward, adjoint=rso.adjoint)
    return pr, lab, res
