"""Snapshot tracking on the device (-m gpu): the load and cost kernels (kernels_obs.hip), the adjoint sweeps with
observations in every kernel regime, their two corner cases against the existing sweeps bit for bit, unobserved levels,
PGD, the reaction variant, error paths and the example -- against the CPU loop of snapshots_oracle.py.

Device data is in the context's DoF order (FEniCS or vertex order), the oracle's in FEniCS DoF order; ``_Order`` converts.
Worst errors measured on an MI355X are in the docstrings of the tests that print them."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import reaction_source_oracle as rso
import snapshots_oracle as so
from regime_helpers import regime_knobs_default

pytestmark = pytest.mark.gpu

ADJ_TOL = 1e-9          # tests/test_gpu_systems_regimes.py
EPS = np.finfo(float).eps
OM = np.pi / 40


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_MESH = {}


def _oracle(N, a1=-1.0, a2=1.0):
    """(mesh, assembler) of the oracle with N nodes per side, one mesh kept at a time (the cases come grouped by N)"""
    key = (N, a1, a2)
    if key not in _MESH:
        from oracle.mesh import SquareMesh
        from oracle.assembly import P1Assembler
        mesh = SquareMesh(a1, a2, N - 1)
        _MESH.clear()
        _MESH[key] = (mesh, P1Assembler(mesh))
    return _MESH[key]


class _Order:
    def __init__(self, mesh, vertex):
        self.n, self.v2d, self.vertex = mesh.nodes, mesh.vertex_to_dof, vertex

    def to_dev(self, a):
        a = np.asarray(a, dtype=np.float64)
        return np.ascontiguousarray(a.reshape(-1, self.n)[:, self.v2d]).reshape(a.shape) if self.vertex else a.copy()

    def from_dev(self, a):
        if not self.vertex:
            return np.array(a)
        o = np.empty((a.size // self.n, self.n))
        o[:, self.v2d] = a.reshape(-1, self.n)
        return o.reshape(a.shape)


def _fields(mesh, count, seed):
    """``count`` nodal fields in FEniCS DoF order: smooth + rough"""
    rng = np.random.default_rng(seed)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    k = rng.uniform(0.5, 3.0, (count, 2))
    return np.sin(k[:, :1] * x + 0.3) * np.cos(k[:, 1:] * y - 0.2) + 0.2 * rng.random((count, mesh.nodes))


def _window(mesh):
    """a window that is 0 on the left half of the domain and varies on the right"""
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    return np.where(x > 0, 0.5 + x * (1 + 0.5 * np.sin(3 * y)), 0.0)


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("windowed", [False, True], ids=["M", "window"])
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("N", [5, 21])
def test_obs_load_kernel(hp, solvers, N, vertex, windowed):
    """k_obs_load alone against the CPU weighted-mass product, batch 3 and each member alone (the same bits), and an
    unobserved level with NaN operands (exact zeros).  Bound: a row is a sum of <= 19 products of <= 4 factors, each term
    and each partial sum rounded once -- 32 eps of the row's sum of absolute terms, for either side's summation order."""
    mesh, asm = _oracle(N)
    od = _Order(mesh, vertex)
    n, B, dt = mesh.nodes, 3, 2.5e-3
    a, b = _fields(mesh, B, [N, 1]), _fields(mesh, B, [N, 2])
    w = _window(mesh) if windowed else None
    theta = np.array([0.0, 0.7 * dt, 0.0, 1.0])
    Mw = so.weighted_mass(asm, w) if windowed else asm.mass()
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), 3, dt, batch=B,
                                  order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
    ctx = prob.ctx
    try:
        da, db, dth, out = ctx.array(od.to_dev(a).ravel()), ctx.array(od.to_dev(b).ravel()), ctx.array(theta), ctx.zeros(B * n)
        dw = None if w is None else ctx.array(od.to_dev(w))
        worst = 0.0
        for level in (1, 3):
            ctx.obs_load(da, db, dth, level, dt, out, window=dw, batch=B)
            got = out.download().reshape(B, n)
            for m in range(B):
                ctx.obs_load(da.ptr + 8 * m * n, db.ptr + 8 * m * n, dth, level, dt, out, window=dw, batch=1)
                assert np.array_equal(out.download()[:n], got[m])
                ref = (theta[level] / dt) * (Mw @ (a[m] - b[m]))
                bound = 32 * EPS * (theta[level] / dt) * (abs(Mw) @ np.abs(a[m] - b[m]))
                err = np.abs(od.from_dev(got[m]) - ref)
                assert np.all(err <= bound), (err / np.maximum(bound, 1e-300)).max()
                worst = max(worst, (err / np.maximum(bound / 32, 1e-300)).max())
            if windowed:                                    # rows whose whole stencil lies where omega = 0
                M = asm.mass()
                dark = np.array([not w[M.indices[M.indptr[i]:M.indptr[i + 1]]].any() for i in range(n)])
                assert dark.any() and not od.from_dev(got[0])[dark].any()
        print(f"[snapshots] k_obs_load N={N} worst error {worst:.2f} eps of the row's absolute sum")
        nan = ctx.array(np.full(B * n, np.nan))
        out.upload(np.full(B * n, 7.0))
        ctx.obs_load(nan, nan, dth, 2, dt, out, window=dw, batch=B)        # theta[2] == 0: operands unread
        res = out.download()
        assert not res.any() and not np.signbit(res).any()
    finally:
        prob.close()


@pytest.mark.parametrize("windowed", [False, True], ids=["M", "window"])
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("N", [5, 21])
def test_obs_cost_kernel(hp, solvers, N, vertex, windowed):
    """k_obs_cost against the CPU sum; a member costed in a batch of 7 and alone: identical bits; NaN at the levels of
    zero weight.  Bound: the sum has T = 7 n L terms (L observed levels); any summation order of T rounded terms is
    within T eps of the sum of their absolute values -- twice that for the two sides."""
    mesh, asm = _oracle(N)
    od = _Order(mesh, vertex)
    n, Nt, B = mesh.nodes, 6, 7
    tl = (Nt + 1) * n
    obs = solvers.Observations(Nt, [2, 6], [0.5, 2.0], window=_window(mesh) if windowed else None)
    u = _fields(mesh, B * (Nt + 1), [N, 3]).reshape(B, tl)
    uh = _fields(mesh, B * (Nt + 1), [N, 4]).reshape(B, tl)
    for lv in np.flatnonzero(obs.cost_w == 0):
        uh[:, lv * n:(lv + 1) * n] = np.nan
    M = asm.mass()
    Mw = so.weighted_mass(asm, obs.window) if windowed else M
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, 1e-3, batch=B,
                                  order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
    ctx = prob.ctx
    try:
        theta, cw, dw = prob.obs_device(solvers.Observations(Nt, [2, 6], [0.5, 2.0],
                                                             window=None if obs.window is None else od.to_dev(obs.window)))
        du, dh = ctx.array(od.to_dev(u.reshape(-1, n)).ravel()), ctx.array(od.to_dev(uh.reshape(-1, n)).ravel())
        J7 = ctx.obs_cost(du, dh, cw, Nt, window=dw, batch=B)
        worst = 0.0
        for m in range(B):
            J1 = ctx.obs_cost(du.ptr + 8 * m * tl, dh.ptr + 8 * m * tl, cw, Nt, window=dw, batch=1)
            assert J1[0] == J7[m]
            ref = so.misfit(asm, M, u[m], uh[m], obs, n)
            absum = 0.5 * sum(obs.cost_w[lv] * (np.abs(u[m] - uh[m])[lv * n:(lv + 1) * n]
                                               @ (abs(Mw) @ np.abs(u[m] - uh[m])[lv * n:(lv + 1) * n])) for lv in (2, 6))
            bound = 2 * (7 * n * 2) * EPS * absum
            assert abs(J7[m] - ref) <= bound, (J7[m], ref, bound)
            worst = max(worst, abs(J7[m] - ref) / ref)
        print(f"[snapshots] k_obs_cost N={N} worst relative error {worst:.2e}")
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ the adjoint sweep
def _member(mesh, Nt, dt, m):
    """Inputs of member m in FEniCS DoF order: a rough control, a smooth state trajectory (the adjoint sweep takes any),
    a target next to it with NaN at every level but 2 and Nt"""
    n = mesh.nodes
    rng = np.random.default_rng([n, m])
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    t = np.arange(Nt + 1)[:, None] * dt
    c = 2.0 * rng.random((Nt + 1) * n)
    u = (np.exp(-10 * ((x + 0.3 - 3 * t) ** 2 + (y - 0.2 + 0.1 * m * t) ** 2)) + 0.05 * rng.random((Nt + 1, n))).ravel()
    uh = np.full((Nt + 1) * n, np.nan)
    for lv in (2, Nt):
        uh[lv * n:(lv + 1) * n] = 0.8 * u[lv * n:(lv + 1) * n] + 0.02 * np.cos(2 * x) * np.sin(y + m)
    return c, u, uh


_ADJ = {}


def _adjoint_oracle(N, Nt, dt, obs, m):
    key = (N, Nt, m)
    if key not in _ADJ:
        from oracle import traj as otraj
        mesh, asm = _oracle(N)
        if any(k[0] != N for k in _ADJ):
            _ADJ.clear()
        c, u, uh = _member(mesh, Nt, dt, m)
        _ADJ[key] = so.adjoint(otraj.SolidBody(asm, om=OM), c, u, uh, obs, mesh.nodes, Nt, dt)
    return _ADJ[key]


REGIMES = [
    pytest.param(21, 1, "MESH", id="N21-B1-one-workgroup"),
    pytest.param(46, 1, "TILE32", id="N46-B1"),
    pytest.param(81, 14, "PATCH64", id="N81-B14"),
    pytest.param(81, 64, "MESH", id="N81-B64-large-batch-mesh-step"),
    pytest.param(129, 6, "PATCH64", id="N129-B6"),
]


@pytest.mark.parametrize("N, B, regime", REGIMES)
def test_adjoint_obs_in_every_regime(hp, solvers, N, B, regime):
    """femfct_solidbody_adjoint_obs in vertex order, snapshots at the interior level 2 (weight 0.7) and the last level
    (weight 1.3), NaN in every other level of the target, B members with their own data: the first, middle and last
    member against the CPU loop, ADJ_TOL.  Worst measured: see the printed line."""
    Nt = 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    members = sorted({0, B // 2, B - 1})
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, batch=B, order=hp.ORDER_VERTEX)
    ctx = prob.ctx
    try:
        if regime_knobs_default():
            assert ctx.kernel_regime(B) == getattr(hp._lib, "REGIME_" + regime)
        data = [_member(mesh, Nt, dt, m) for m in range(B)]
        dc, du, dh = (ctx.array(np.concatenate([od.to_dev(d[k].reshape(-1, n)).ravel() for d in data])) for k in range(3))
        dp = ctx.zeros(B * tl)
        prob.adjoint(dc, du, dh, dp, "snapshots", batch=B, obs=obs)
        log = prob.solver_log(B)
        p = dp.download().reshape(B, tl)
    finally:
        prob.close()
    assert np.isfinite(p).all()
    assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET)
    errs = [rel(od.from_dev(p[m]), _adjoint_oracle(N, Nt, dt, obs, m)) for m in members]
    print(f"[snapshots] adjoint N={N} B={B}: worst rel l2 error vs the CPU loop {max(errs):.3e}")
    assert max(errs) < ADJ_TOL, errs


def _corner_inputs(hp, N, Nt, dt, B):
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    n = mesh.nodes
    data = [_member(mesh, Nt, dt, m) for m in range(B)]
    c = np.concatenate([od.to_dev(d[0].reshape(-1, n)).ravel() for d in data])
    u = np.concatenate([od.to_dev(d[1].reshape(-1, n)).ravel() for d in data])
    rng = np.random.default_rng(N)
    return n, c, u, 0.9 * u + 0.01 * rng.random(u.size)


@pytest.mark.parametrize("N", [21, 46])
def test_corner_cases_equal_the_existing_sweeps_bitwise(hp, solvers, N):
    """(tau, theta) = (1, 0) is femfct_solidbody_adjoint(alltime = 0) and (0, dt) is alltime = 1, bit for bit, two members.
    Each sweep runs on a context of its own: the sweep controller keeps the Jacobi budget it learnt from earlier sweeps
    of a context, and the tile kernels return the iterate of the budget's last sweep, so two runs of one and the same
    sweep have the same bits only from the same history."""
    Nt, B = 6, 2
    dt = 1e-3 * 80 / (N - 1)
    n, c, u, uh = _corner_inputs(hp, N, Nt, dt, B)
    tl = (Nt + 1) * n
    uhT = np.concatenate([uh[b * tl + Nt * n:(b + 1) * tl] for b in range(B)])

    def sweep(optim, target, obs=None):
        prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, batch=B, order=hp.ORDER_VERTEX)
        ctx = prob.ctx
        try:
            dp = ctx.zeros(B * tl)
            prob.adjoint(ctx.array(c), ctx.array(u), ctx.array(target), dp, optim, batch=B, obs=obs)
            return dp.download()
        finally:
            prob.close()

    p_fin, p_all = sweep("finaltime", uhT), sweep("alltime", uh)
    assert np.array_equal(sweep("finaltime", uhT), p_fin)                   # (the premise: equal histories, equal bits)
    assert np.array_equal(sweep("snapshots", uh, solvers.Observations.finaltime(Nt)), p_fin)
    assert np.array_equal(sweep("snapshots", uh, solvers.Observations.alltime(Nt, dt)), p_all)
    assert p_fin.any() and p_all.any() and not np.array_equal(p_fin, p_all)


def test_unobserved_levels_are_not_read_and_observed_nan_fails(hp, solvers):
    """NaN in the unobserved levels of the target leaves p and the cost unchanged bit for bit; NaN at an observed level
    (interior, last) fails the solve with NotConverged."""
    N, Nt = 21, 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    c, u, uh_nan = _member(mesh, Nt, dt, 0)
    uh_fin = np.where(np.isnan(uh_nan), 0.3, uh_nan)
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    new = lambda: solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    out = []
    for uh in (uh_nan, uh_fin):                 # a context each: the same history of sweeps (see the corner cases)
        prob = new()
        ctx = prob.ctx
        try:
            dc, du, dp, dh = ctx.array(od.to_dev(c)), ctx.array(od.to_dev(u)), ctx.zeros(tl), ctx.array(od.to_dev(uh))
            prob.adjoint(dc, du, dh, dp, "snapshots", batch=1, obs=obs)
            out.append((dp.download(), prob.cost(du, dh, dc, 0.1, "snapshots", batch=1, obs=obs)[0]))
        finally:
            prob.close()
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1])
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    prob = new()
    ctx = prob.ctx
    try:
        dc, du, dp = ctx.array(od.to_dev(c)), ctx.array(od.to_dev(u)), ctx.zeros(tl)
        for lv in (2, Nt):
            bad = uh_fin.copy()
            bad[lv * n + n // 2] = np.nan
            with pytest.raises(hp._lib.NotConverged):
                prob.adjoint(dc, du, ctx.array(od.to_dev(bad)), dp.zero(), "snapshots", batch=1, obs=obs)
        prob.adjoint(dc, du, ctx.array(od.to_dev(uh_fin)), dp.zero(), "snapshots", batch=1, obs=obs)     # healthy again
        assert rel(dp.download(), out[0][0]) < 1e-11            # (another history of sweeps: the solver tolerance, not bits)
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ PGD
@pytest.fixture(scope="module")
def pgd_case():
    """N = 21, 20 steps, snapshots at levels 10 and 20, three iterations, on the CPU: every Armijo margin >= 1e-8"""
    from oracle import traj as otraj
    N, Nt, dt, beta = 21, 20, 2e-3, 0.05
    mesh, asm = _oracle(N)
    n = mesh.nodes
    sb = otraj.SolidBody(asm, om=OM)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
    obs_levels = [10, 20]
    tgt = np.zeros((Nt + 1) * n)
    tgt[:n] = u0
    t = np.arange(Nt + 1)[:, None] * dt
    otraj.solidbody_forward(sb, (1.5 + np.sin(2 * x)[None] * np.cos(y + 5 * t)).ravel(), tgt, n, Nt, dt)
    uhat = np.full_like(tgt, np.nan)
    for lv in obs_levels:
        uhat[lv * n:(lv + 1) * n] = tgt[lv * n:(lv + 1) * n]
    return dict(N=N, Nt=Nt, dt=dt, beta=beta, n=n, sb=sb, u0=u0, uhat=uhat, levels=obs_levels, mesh=mesh)


def test_pgd_snapshots_matches_the_cpu_loop(hp, solvers, pgd_case):
    """pgd_solidbody_snapshots against the CPU loop: the same Armijo trial counts, costs to 1e-10 relative."""
    k = pgd_case
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    obs = solvers.Observations(Nt, k["levels"])
    c0 = np.full((Nt + 1) * n, 0.5)
    uo, po, co, ho = so.pgd_loop(k["sb"], k["u0"], k["uhat"], obs, c0, k["beta"], 0.0, 5.0, 3, n, Nt, dt, max_armijo=6)
    print(f"[snapshots] PGD on the CPU: costs {ho['cost']}, trials {ho['armijo_k']}, smallest margin {ho['armijo_margin_min']:.3e}")
    assert ho["armijo_margin_min"] >= 1e-8          # no accept / reject decision hangs on rounding
    od = _Order(k["mesh"], True)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    try:
        u, p, c, h = solvers.pgd_solidbody_snapshots(prob, od.to_dev(k["u0"]), od.to_dev(k["uhat"]), obs, od.to_dev(c0),
                                                     k["beta"], 0.0, 5.0, 3, max_armijo=6)
    finally:
        prob.close()
    assert h["armijo_k"] == ho["armijo_k"]
    errs = [abs(a - b) / abs(b) for a, b in zip(h["cost"], ho["cost"])]
    print(f"[snapshots] PGD device vs CPU: cost errors {errs}, state {rel(od.from_dev(u), uo):.2e}, control {rel(od.from_dev(c), co):.2e}")
    assert max(errs) <= 1e-10
    assert rel(od.from_dev(u), uo) < ADJ_TOL and rel(od.from_dev(c), co) < ADJ_TOL


# ------------------------------------------------------------------------------------------------ reaction variant
def test_reaction_variant_against_the_cpu_loop(hp, solvers):
    """LinearReactionSourceControl.adjoint_state(optim="snapshots") at N = 21 with g != 0, and its two corners bitwise."""
    N, Nt, eps = 21, 6, 1e-3
    mesh, asm = _oracle(N, 0.0, 1.0)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    dt = 1e-3
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    t = np.arange(Nt + 1)[:, None] * dt
    g = (1.0 + 0.5 * np.sin(3 * x)[None] * np.cos(2 * y + 40 * t)).ravel()
    wind = solvers.finaltime_exact_wind()
    rs = rso.ReactionSource(asm, g, eps=eps, wind=wind, wind_rule=rso.DEVICE_WIND_RULE)
    _, u, uh = _member(mesh, Nt, dt, 0)
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    po = so.adjoint(rs, None, u, uh, obs, n, Nt, dt, Mg=rs.Mg, A_p=rs.A_p)
    uh_fin = np.where(np.isnan(uh), 0.3, uh)

    def sweep(optim, target, o=None):           # a context each: the same history of sweeps (see the corner cases)
        prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind, g, eps=eps)
        ctx = prob.ctx
        try:
            dp = ctx.zeros(tl)
            prob.adjoint_state(ctx.array(u), ctx.array(target), dp, optim, batch=1, obs=o)
            return dp.download()
        finally:
            prob.close()

    err = rel(sweep("snapshots", uh, obs), po)
    print(f"[snapshots] reaction variant N={N}: rel l2 error vs the CPU loop {err:.3e}")
    assert err < ADJ_TOL
    assert np.array_equal(sweep("snapshots", uh_fin, solvers.Observations.finaltime(Nt)), sweep("finaltime", uh_fin[Nt * n:]))
    assert np.array_equal(sweep("snapshots", uh_fin, solvers.Observations.alltime(Nt, dt)), sweep("alltime", uh_fin))


def test_source_control_pgd_snapshots_runs_resolve_only(hp, solvers):
    """pgd_source_control(optim="snapshots", increment="resolve") descends; increment="linear" refuses the mode."""
    N, Nt, dt = 21, 6, 2e-3
    mesh, _ = _oracle(N, 0.0, 1.0)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    uhat = np.full(tl, np.nan)
    for lv in (3, Nt):
        uhat[lv * n:(lv + 1) * n] = 0.2 * np.sin(np.pi * x) * np.sin(np.pi * y) * lv / Nt
    obs = solvers.Observations(Nt, [3, Nt])
    from oracle.traj import exact_velocity
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, exact_velocity)
    try:
        kw = dict(beta=1e-3, c_lower=0.0, c_upper=50.0, optim="snapshots", obs=obs, max_armijo=5, max_iters=3, tol=0.0)
        with pytest.raises(ValueError):
            solvers.pgd_source_control(prob, np.zeros(n), uhat, np.zeros(tl), increment="linear", **kw)
        u, p, c, h = solvers.pgd_source_control(prob, np.zeros(n), uhat, np.zeros(tl), increment="resolve", **kw)
        assert h["iterations"] == 3 and np.isfinite(h["cost"]).all()
        assert h["cost"][-1] < h["cost_state"][0]
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ error paths, example
def test_error_paths(hp, solvers):
    N, Nt, dt = 5, 4, 1e-3
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt)
    ctx, n = prob.ctx, prob.n
    try:
        c, u, uh, p = ctx.zeros(prob.tlen), ctx.zeros(prob.tlen), ctx.zeros(prob.tlen), ctx.zeros(prob.tlen)
        with pytest.raises(hp._lib.FemFctValueError):           # a null theta
            ctx.solidbody_adjoint_obs(prob.Arot, c, u, uh, None, 1.0, None, p, Nt, dt)
        with pytest.raises(hp._lib.FemFctValueError):
            ctx.obs_load(u, uh, None, 0, dt, p)
        with pytest.raises(hp._lib.FemFctValueError):
            ctx.obs_cost(u, uh, None, Nt)
        with pytest.raises(ValueError):                         # a window of the wrong length
            prob.adjoint(c, u, uh, p, "snapshots", batch=1, obs=solvers.Observations(Nt, [2], window=np.ones(n + 1)))
        with pytest.raises(ValueError):                         # observations of another number of steps
            prob.adjoint(c, u, uh, p, "snapshots", batch=1, obs=solvers.Observations(Nt + 1, [2]))
        with pytest.raises(ValueError):                         # optim="snapshots" without obs
            prob.adjoint(c, u, uh, p, "snapshots", batch=1)
        with pytest.raises(ValueError):
            prob.cost(u, uh, c, 0.1, "snapshots", batch=1)
        with pytest.raises(ValueError):
            solvers.pgd_solidbody(prob, np.zeros(n), np.zeros(prob.tlen), np.zeros(prob.tlen), 0.1, 0.0, 1.0, 1,
                                  optim="snapshots")
        prob.adjoint(c, u, uh, p, "snapshots", batch=1, obs=solvers.Observations(Nt, [2, Nt]))      # still usable
    finally:
        prob.close()


def test_example_runs_at_a_reduced_size():
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "solidbody_snapshots_pdeco.py"), "--iters", "2", "--steps", "12",
                          "--trials", "4"], capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "snapshots at levels [6, 12] of 12: 2 PGD iterations in" in out.stdout
    costs = [float(ln.split("J =")[1].split()[0]) for ln in out.stdout.splitlines() if ln.startswith("it ")]
    assert len(costs) == 2 and np.isfinite(costs).all()
