"""State bounds on the device (-m gpu): the load and cost kernels (kernels_bounds.hip), the adjoint sweeps with bounds in
every kernel regime, inactive bounds against the existing sweeps bit for bit, the graph key, the loops, NaN, error paths
and the example -- against the CPU loop of state_bounds_oracle.py.

Device data is in the context's DoF order (FEniCS or vertex order), the oracle's in FEniCS DoF order; ``_Order`` converts.
The inputs, helpers and bars are those of test_gpu_snapshots.py."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import reaction_source_oracle as rso
import snapshots_oracle as so
import state_bounds_oracle as sbo
from regime_helpers import regime_knobs_default
from test_gpu_snapshots import ADJ_TOL, EPS, OM, REGIMES, _Order, _corner_inputs, _fields, _member, _oracle, _window, rel

pytestmark = pytest.mark.gpu

LO, HI, GAMMA = 0.02, 0.3, 200.0        # the sweeps' two-sided bounds: ~35 % of the pairs of _member's states violate them


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def _dev_bounds(solvers, od, b):
    """the bounds ``b`` (FEniCS DoF order) with their nodal fields in the device's order"""
    lo, hi, w = b.nodal(od.n)
    f = lambda a: None if a is None else od.to_dev(a)
    lv = b.levels
    return solvers.StateBounds(b.num_steps, lower=f(lo), upper=f(hi), gamma=b.gamma, levels=lv,
                               weights=None if b._per_dt else b._level_w[lv], window=f(w))


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("react", [False, True], ids=["plain", "react"])
@pytest.mark.parametrize("windowed", [False, True], ids=["M", "windows"])
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("N", [5, 21])
def test_bound_load_kernel(hp, solvers, N, vertex, windowed, react):
    """k_bound_load alone against NumPy, batch 3 and each member alone (the same bits), at a level with both parts, one
    without a penalty and one without a tracking part (NaN target: unread).  Bound: the 32 eps of test_obs_load_kernel
    on the row's sum of absolute tracking and reaction terms, plus 8 eps |penalty term| -- the term is v with one
    rounding, four products and the subtraction.  Inactive bounds (upper = +inf; gamma = 0): femfct_obs_load's bits --
    in the cases without a reaction part, which femfct_obs_load does not take; with one the bits are compared on the
    whole sweep (test_reaction_variant_against_the_cpu_loop).  NaN in u at a penalised, unobserved level: a NaN load."""
    mesh, asm = _oracle(N)
    od = _Order(mesh, vertex)
    n, B, dt, gamma = mesh.nodes, 3, 2.5e-3, 40.0
    uh, u, x = _fields(mesh, B, [N, 1]), _fields(mesh, B, [N, 2]), _fields(mesh, B, [N, 5])
    g = _fields(mesh, 1, [N, 6])[0] if react else None
    w = _window(mesh) if windowed else None
    ws = (0.3 + _window(mesh)[::-1]) * (mesh.x[mesh.dof_to_vertex] < 0.6) if windowed else None
    lo, hi = -0.1 + 0.1 * _fields(mesh, 1, [N, 7])[0], np.full(n, 0.3)
    theta = np.array([0.0, 0.7 * dt, 1.0, 0.0])
    sigma = np.array([0.0, 0.4 * dt, 0.0, 1.5])
    M = asm.mass()
    Mw = so.weighted_mass(asm, w) if windowed else M
    Mg = so.weighted_mass(asm, g) if react else None
    ml = sbo.lumped(M)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), 3, dt, batch=B,
                                  order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
    ctx = prob.ctx
    try:
        up = lambda a: None if a is None else ctx.array(od.to_dev(a).ravel())
        dh, du, dx, dg, dw, dws, dlo, dhi = (up(a) for a in (uh, u, x, g, w, ws, lo, hi))
        dth, dsg, out = ctx.array(theta), ctx.array(sigma), ctx.zeros(B * n)
        nan = ctx.array(np.full(B * n, np.nan))
        # the term's roundings are counted from the kernel's inputs, the context's lumped mass among them: the reference
        # takes its bits.  They are the CPU's row sums to rounding: a row of the assembled M sums <= 18 element integrals,
        # each a rounded quadrature sum -- 32 eps, the bound of a load row above (all terms positive)
        ml_cpu, ml = ml, od.from_dev(ctx.empty(n).copy_from(ctx.lumped_mass, n).download())
        assert np.all(np.abs(ml - ml_cpu) <= 32 * EPS * ml_cpu)
        kw = dict(window=dw, g=dg, x=dx if react else None, window_s=dws)
        worst = 0.0
        for level in (1, 2, 3):
            tgt = nan if theta[level] == 0 else dh              # theta == 0: the target is not read
            ctx.bound_load(tgt, du, dth, dsg, level, dt, dlo, dhi, gamma, out, batch=B, **kw)
            got = out.download().reshape(B, n)
            for m in range(B):
                ctx.bound_load(tgt.ptr + 8 * m * n, du.ptr + 8 * m * n, dth, dsg, level, dt, dlo, dhi, gamma, out,
                               batch=1, **{**kw, "x": dx.ptr + 8 * m * n if react else None})
                assert np.array_equal(out.download()[:n], got[m])
                s = theta[level] / dt
                ref, absum = s * (Mw @ (uh[m] - u[m])), s * (abs(Mw) @ np.abs(uh[m] - u[m]))
                if react:
                    ref, absum = ref - Mg @ x[m], absum + abs(Mg) @ np.abs(x[m])
                term = (sigma[level] / dt) * gamma * ml * (1.0 if ws is None else ws) * sbo.violation(u[m], lo, hi)
                ref = ref - term
                bound = 32 * EPS * absum + 8 * EPS * np.abs(term)
                err = np.abs(od.from_dev(got[m]) - ref)
                assert np.all(err <= bound), (level, (err / np.maximum(bound, 1e-300)).max())
                worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
                if level != 2:
                    assert np.count_nonzero(term) > n // 10     # (the case has a penalty to check)
        print(f"[state bounds] k_bound_load N={N}: worst error {worst:.3f} of the bound")
        if not react:                                           # inactive bounds: femfct_obs_load's bits
            ref_out = ctx.zeros(B * n)
            inf = ctx.array(np.full(n, np.inf))
            ctx.obs_load(dh, du, dth, 1, dt, ref_out, window=dw, batch=B)
            ctx.bound_load(dh, du, dth, dsg, 1, dt, None, inf, gamma, out, window=dw, window_s=dws, batch=B)
            assert np.array_equal(out.download(), ref_out.download()) and ref_out.download().any()
            ctx.bound_load(dh, du, dth, dsg, 1, dt, dlo, dhi, 0.0, out, window=dw, window_s=dws, batch=B)
            assert np.array_equal(out.download(), ref_out.download())
        bad = od.to_dev(u).ravel()
        bad[n + n // 2] = np.nan                                # member 1, level 3: penalised, not observed
        ctx.bound_load(nan, ctx.array(bad), dth, dsg, 3, dt, dlo, dhi, gamma, out, batch=B,
                       **{**kw, "window_s": None})
        res = out.download().reshape(B, n)
        assert np.isnan(res[1, n // 2]) and np.isfinite(res[0]).all() and np.isfinite(res[2]).all()
        assert np.count_nonzero(np.isnan(res[1])) == 1
    finally:
        prob.close()


@pytest.mark.parametrize("windowed", [False, True], ids=["all", "window"])
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("N", [5, 21])
def test_bound_cost_kernel(hp, solvers, N, vertex, windowed):
    """k_bound_cost against NumPy: P within twice (T + 8) eps of the sum of its absolute terms, T = n L terms (L penalised
    levels; the derivation of test_obs_cost_kernel, 8 for the roundings inside a term), the largest |v| bit for bit and the
    count exactly; a member in a batch of 7 and alone: identical bits.  NaN at the levels of zero weight is not read."""
    mesh, asm = _oracle(N)
    od = _Order(mesh, vertex)
    n, Nt, B, dt = mesh.nodes, 6, 7, 1e-3
    tl = (Nt + 1) * n
    w = _window(mesh) if windowed else None
    b = solvers.StateBounds(Nt, lower=-0.1 + 0.1 * _fields(mesh, 1, [N, 7])[0], upper=0.3, gamma=30.0, levels=[2, 5, 6],
                            weights=[0.5, 1.0, 2.0], window=w)
    u = _fields(mesh, B * (Nt + 1), [N, 3]).reshape(B, tl)
    for lv in np.flatnonzero(b.sigma(dt) == 0):
        u[:, lv * n:(lv + 1) * n] = np.nan
    M = asm.mass()
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, batch=B,
                                  order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
    ctx = prob.ctx
    try:
        bd = _dev_bounds(solvers, od, b)
        sg, lo, hi, win = prob.bounds_device(bd)
        du = ctx.array(od.to_dev(u.reshape(-1, n)).ravel())
        S7 = ctx.bound_cost(du, sg, lo, hi, b.gamma, Nt, window_s=win, batch=B)
        P7, vmax7, frac7 = prob.bound_stats(du, bd, batch=B)
        assert np.array_equal(P7, S7[:, 0]) and np.array_equal(vmax7, S7[:, 1])
        worst = 0.0
        for m in range(B):
            S1 = ctx.bound_cost(du.ptr + 8 * m * tl, sg, lo, hi, b.gamma, Nt, window_s=win, batch=1)
            assert np.array_equal(S1[0], S7[m])
            P, vmax, count, frac = sbo.stats(M, u[m], b, n, dt)
            bound = 2 * (n * 3 + 8) * EPS * P               # (every term is >= 0: the sum of absolute terms is P)
            assert abs(S7[m, 0] - P) <= bound, (S7[m, 0], P, bound)
            assert S7[m, 1] == vmax and S7[m, 2] == count and frac7[m] == frac and 0 < count < b.pairs(n, dt)
            worst = max(worst, abs(S7[m, 0] - P) / P)
        print(f"[state bounds] k_bound_cost N={N}: worst relative error {worst:.2e}")
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ the adjoint sweep
def _violated_fraction(u, n, Nt, lo, hi):
    v = sbo.violation(u.reshape(Nt + 1, n)[1:], lo, hi)
    return np.count_nonzero(v) / v.size


_ADJ = {}


def _adjoint_oracle(N, Nt, dt, obs, bounds, m):
    key = (N, Nt, m, bounds.gamma)
    if key not in _ADJ:
        from oracle import traj as otraj
        mesh, asm = _oracle(N)
        if any(k[0] != N for k in _ADJ):
            _ADJ.clear()
        c, u, uh = _member(mesh, Nt, dt, m)
        frac = _violated_fraction(u, mesh.nodes, Nt, LO, HI)
        assert 0.05 <= frac <= 0.6, frac                    # a condition on the inputs
        _ADJ[key] = sbo.adjoint(otraj.SolidBody(asm, om=OM), c, u, uh, obs, bounds, mesh.nodes, Nt, dt)
    return _ADJ[key]


@pytest.mark.parametrize("N, B, regime", REGIMES)
def test_adjoint_bounds_in_every_regime(hp, solvers, N, B, regime):
    """femfct_solidbody_adjoint_bounds in vertex order: the sweep of test_adjoint_obs_in_every_regime with two-sided
    bounds that between 5 % and 60 % of the penalised pairs violate (asserted on the CPU), B members with their own
    data: the first, middle and last member against the CPU loop, ADJ_TOL."""
    Nt = 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    bounds = solvers.StateBounds(Nt, lower=LO, upper=HI, gamma=GAMMA)
    members = sorted({0, B // 2, B - 1})
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, batch=B, order=hp.ORDER_VERTEX)
    ctx = prob.ctx
    try:
        if regime_knobs_default():
            assert ctx.kernel_regime(B) == getattr(hp._lib, "REGIME_" + regime)
        data = [_member(mesh, Nt, dt, m) for m in range(B)]
        dc, du, dh = (ctx.array(np.concatenate([od.to_dev(d[k].reshape(-1, n)).ravel() for d in data])) for k in range(3))
        dp = ctx.zeros(B * tl)
        prob.adjoint(dc, du, dh, dp, "snapshots", batch=B, obs=obs, state_bounds=bounds)
        log = prob.solver_log(B)
        p = dp.download().reshape(B, tl)
    finally:
        prob.close()
    assert np.isfinite(p).all()
    assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET)
    errs = [rel(od.from_dev(p[m]), _adjoint_oracle(N, Nt, dt, obs, bounds, m)) for m in members]
    print(f"[state bounds] adjoint N={N} B={B}: worst rel l2 error vs the CPU loop {max(errs):.3e}")
    assert max(errs) < ADJ_TOL, errs


def test_graph_key_holds_gamma(hp, solvers):
    """One context, the same buffers, two sweeps that differ in gamma alone: each matches its CPU result, and the two
    differ (a graph replayed with the first gamma baked in would give the first result twice)."""
    N, Nt = 21, 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    tl = (Nt + 1) * mesh.nodes
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    b5 = solvers.StateBounds(Nt, lower=LO, upper=HI, gamma=5.0)
    c, u, uh = _member(mesh, Nt, dt, 0)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    ctx = prob.ctx
    try:
        dc, du, dh, dp = ctx.array(od.to_dev(c)), ctx.array(od.to_dev(u)), ctx.array(od.to_dev(uh)), ctx.zeros(tl)
        got = []
        for b in (b5, b5.with_gamma(50.0)):
            prob.adjoint(dc, du, dh, dp.zero(), "snapshots", batch=1, obs=obs, state_bounds=b)
            got.append(od.from_dev(dp.download()))
            assert rel(got[-1], _adjoint_oracle(N, Nt, dt, obs, b, 0)) < ADJ_TOL
    finally:
        prob.close()
    assert rel(got[0], got[1]) > 1e-2


def test_reaction_variant_against_the_cpu_loop(hp, solvers):
    """LinearReactionSourceControl.adjoint_state(state_bounds=...) at N = 21 with g != 0 against the CPU loop; with
    bounds that nothing violates, and with gamma = 0, the sweep without ``state_bounds`` bit for bit (a context per sweep:
    the same history, see test_corner_cases_equal_the_existing_sweeps_bitwise)."""
    N, Nt, eps, dt = 21, 6, 1e-3, 1e-3
    mesh, asm = _oracle(N, 0.0, 1.0)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    t = np.arange(Nt + 1)[:, None] * dt
    g = (1.0 + 0.5 * np.sin(3 * x)[None] * np.cos(2 * y + 40 * t)).ravel()
    wind = solvers.finaltime_exact_wind()
    rs = rso.ReactionSource(asm, g, eps=eps, wind=wind, wind_rule=rso.DEVICE_WIND_RULE)
    _, u, uh = _member(mesh, Nt, dt, 0)
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    bounds = solvers.StateBounds(Nt, lower=LO, upper=HI, gamma=GAMMA, window=0.5 + x)
    frac = _violated_fraction(u, n, Nt, LO, HI)
    assert 0.05 <= frac <= 0.6, frac
    po = sbo.adjoint(rs, None, u, uh, obs, bounds, n, Nt, dt, Mg=rs.Mg, A_p=rs.A_p)
    assert rel(po, so.adjoint(rs, None, u, uh, obs, n, Nt, dt, Mg=rs.Mg, A_p=rs.A_p)) > 1e-2     # (the bounds act)

    def sweep(kw):
        prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind, g, eps=eps)
        ctx = prob.ctx
        try:
            dp = ctx.zeros(tl)
            prob.adjoint_state(ctx.array(u), ctx.array(uh), dp, "snapshots", batch=1, obs=obs, **kw)
            return dp.download()
        finally:
            prob.close()

    err = rel(sweep(dict(state_bounds=bounds)), po)
    print(f"[state bounds] reaction variant N={N}: rel l2 error vs the CPU loop {err:.3e}")
    assert err < ADJ_TOL
    p_obs = sweep({})
    assert p_obs.any()
    assert np.array_equal(sweep(dict(state_bounds=solvers.StateBounds(Nt, lower=-50.0, upper=50.0, gamma=GAMMA))), p_obs)
    assert np.array_equal(sweep(dict(state_bounds=bounds.with_gamma(0.0))), p_obs)


def test_unpenalised_levels_are_not_read(hp, solvers):
    """Bounds whose levels leave out the last one, under observations that leave it out too: u_Nt is read by neither the
    terminal condition nor a load, so a NaN there leaves p bit for bit (a context per sweep), and p has the CPU loop's
    values; so it is with a NaN at an interior level that is neither penalised nor observed."""
    N, Nt = 21, 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, asm = _oracle(N)
    od = _Order(mesh, True)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    c, u, uh = _member(mesh, Nt, dt, 0)
    obs = solvers.Observations(Nt, [2])
    bounds = solvers.StateBounds(Nt, lower=LO, upper=HI, gamma=GAMMA, levels=[1, 2, 4, 5])
    assert obs.tau == 0.0 and bounds.tau_s(dt) == 0.0 and bounds.sigma(dt)[3] == 0.0
    holes = u.copy()
    holes[Nt * n:] = np.nan
    holes[3 * n:4 * n] = np.nan

    def sweep(state):
        prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
        ctx = prob.ctx
        try:
            dp = ctx.zeros(tl)
            prob.adjoint(ctx.array(od.to_dev(c)), ctx.array(od.to_dev(state)), ctx.array(od.to_dev(uh)), dp, "snapshots",
                         batch=1, obs=obs, state_bounds=bounds)
            return dp.download()
        finally:
            prob.close()

    p_full, p_holes = sweep(u), sweep(holes)
    assert np.isfinite(p_holes).all() and np.array_equal(p_holes, p_full)
    assert not p_full[Nt * n:].any() and p_full[:5 * n].any()
    from oracle import traj as otraj
    po = sbo.adjoint(otraj.SolidBody(asm, om=OM), c, holes, uh, obs, bounds, n, Nt, dt)
    assert rel(od.from_dev(p_full), po) < ADJ_TOL


# ------------------------------------------------------------------------------------------------ inactive bounds
@pytest.mark.parametrize("N", [21, 46])
def test_inactive_bounds_equal_the_existing_code_bitwise(hp, solvers, N):
    """With bounds that nothing violates the adjoint and the cost of every mode, and a 3-iteration pgd_solidbody history,
    equal the run without ``state_bounds`` bit for bit.  A context per run: the same history of sweeps (see
    test_corner_cases_equal_the_existing_sweeps_bitwise)."""
    Nt, B = 6, 2
    dt = 1e-3 * 80 / (N - 1)
    n, c, u, uh = _corner_inputs(hp, N, Nt, dt, B)
    tl = (Nt + 1) * n
    uhT = np.concatenate([uh[b * tl + Nt * n:(b + 1) * tl] for b in range(B)])
    idle = solvers.StateBounds(Nt, lower=-50.0, upper=np.full(n, 50.0), gamma=GAMMA)
    new = lambda batch: solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, batch=batch,
                                               order=hp.ORDER_VERTEX)

    def sweep(optim, target, obs, kw):
        prob = new(B)
        ctx = prob.ctx
        try:
            dc, du, dh, dp = ctx.array(c), ctx.array(u), ctx.array(target), ctx.zeros(B * tl)
            prob.adjoint(dc, du, dh, dp, optim, batch=B, obs=obs, **kw)
            return dp.download(), prob.cost(du, dh, dc, 0.1, optim, batch=B, obs=obs, **kw)
        finally:
            prob.close()

    for optim, target, obs in (("finaltime", uhT, None), ("alltime", uh, None),
                               ("snapshots", uh, solvers.Observations(Nt, [2, Nt], [0.7, 1.3]))):
        p0, J0 = sweep(optim, target, obs, {})
        p1, J1 = sweep(optim, target, obs, dict(state_bounds=idle))
        assert p0.any() and np.array_equal(p1, p0), optim
        assert np.array_equal(J1, J0), optim

    def loop(kw):
        prob = new(1)
        try:
            return solvers.pgd_solidbody(prob, u[:n], uhT[:n], np.full(tl, 0.5), 0.05, 0.0, 5.0, 3, max_armijo=4, **kw)
        finally:
            prob.close()

    (u0_, p0, c0_, h0), (u1, p1, c1, h1) = loop({}), loop(dict(state_bounds=idle))
    assert np.array_equal(u1, u0_) and np.array_equal(p1, p0) and np.array_equal(c1, c0_)
    assert h1["cost"] == h0["cost"] and h1["armijo_k"] == h0["armijo_k"] and h1["armijo_margin"] == h0["armijo_margin"]
    assert h1["penalty"] == [0.0] * 3 and h1["max_violation"] == [0.0] * 3 and h1["violated_fraction"] == [0.0] * 3
    assert "penalty" not in h0


# ------------------------------------------------------------------------------------------------ the loops
@pytest.fixture(scope="module")
def pgd_case():
    """The case of test_gpu_snapshots.py's PGD test: N = 21, 20 steps, the target a state under another control"""
    from oracle import traj as otraj
    N, Nt, dt, beta = 21, 20, 2e-3, 0.05
    mesh, asm = _oracle(N)
    n = mesh.nodes
    sb = otraj.SolidBody(asm, om=OM)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    u0 = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2))
    tgt = np.zeros((Nt + 1) * n)
    tgt[:n] = u0
    t = np.arange(Nt + 1)[:, None] * dt
    otraj.solidbody_forward(sb, (1.5 + np.sin(2 * x)[None] * np.cos(y + 5 * t)).ravel(), tgt, n, Nt, dt)
    return dict(N=N, Nt=Nt, dt=dt, beta=beta, n=n, sb=sb, u0=u0, tgt=tgt, mesh=mesh)


def _compare_histories(h, ho, pairs):
    assert h["armijo_k"] == ho["armijo_k"]
    close = lambda a, b: np.all(np.abs(np.array(a) - np.array(b)) <= 1e-10 * np.abs(np.array(b)))
    assert close(h["cost"], ho["cost"]), (h["cost"], ho["cost"])
    assert close(h["penalty"], ho["penalty"]) and close(h["max_violation"], ho["max_violation"])
    assert close(h["violated_fraction"], ho["violated_fraction"])
    assert [round(f * pairs) for f in h["violated_fraction"]] == ho["violated"]         # the count, exactly
    assert min(ho["violated"]) > 0


@pytest.mark.parametrize("optim, upper, gamma", [("finaltime", 0.3, 500.0), ("snapshots", 0.5, 2000.0)])
def test_pgd_solidbody_matches_the_cpu_loop(hp, solvers, pgd_case, optim, upper, gamma):
    """pgd_solidbody(state_bounds=...) against the CPU loop, three iterations: the same Armijo trial counts, costs and
    statistics to 1e-10 relative, the count exactly, state and control to ADJ_TOL.  The inputs are chosen so that the
    CPU loop's smallest Armijo margin is >= 1e-8 (asserted).  Measured on the CPU: final-time, u <= 0.3, gamma = 500:
    trials [1, 1, 4], smallest margin 4.5e-5; snapshots, u <= 0.5, gamma = 2000: trials [1, 1, 2], 8.1e-4."""
    k = pgd_case
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    obs = solvers.Observations.finaltime(Nt) if optim == "finaltime" else solvers.Observations(Nt, [10, 20])
    uhat = np.full_like(k["tgt"], np.nan)
    for lv in obs.levels:
        uhat[lv * n:(lv + 1) * n] = k["tgt"][lv * n:(lv + 1) * n]
    bounds = solvers.StateBounds(Nt, upper=upper, gamma=gamma)
    c0 = np.full((Nt + 1) * n, 0.5)
    uo, po, co, ho = sbo.pgd_loop(k["sb"], k["u0"], uhat, obs, bounds, c0, k["beta"], 0.0, 5.0, 3, n, Nt, dt, max_armijo=6)
    print(f"[state bounds] PGD {optim} on the CPU: costs {ho['cost']}, trials {ho['armijo_k']}, smallest margin "
          f"{ho['armijo_margin_min']:.3e}, penalty {ho['penalty']}, violated {ho['violated']}")
    assert ho["armijo_margin_min"] >= 1e-8          # no accept / reject decision hangs on rounding
    od = _Order(k["mesh"], True)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    try:
        target = od.to_dev(uhat[Nt * n:]) if optim == "finaltime" else od.to_dev(uhat)
        u, p, c, h = solvers.pgd_solidbody(prob, od.to_dev(k["u0"]), target, od.to_dev(c0), k["beta"], 0.0, 5.0, 3,
                                           max_armijo=6, optim=optim, obs=obs if optim == "snapshots" else None,
                                           state_bounds=bounds)
    finally:
        prob.close()
    _compare_histories(h, ho, bounds.pairs(n, dt))
    print(f"[state bounds] PGD {optim} device vs CPU: state {rel(od.from_dev(u), uo):.2e}, control {rel(od.from_dev(c), co):.2e}")
    assert rel(od.from_dev(u), uo) < ADJ_TOL and rel(od.from_dev(c), co) < ADJ_TOL


def _source_case():
    from oracle.traj import LinearSource, exact_velocity
    N, Nt, dt = 21, 20, 2e-3
    mesh, asm = _oracle(N, 0.0, 1.0)
    n = mesh.nodes
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    u0 = 0.2 * np.sin(np.pi * x) * np.sin(np.pi * y)            # exceeds the bound 0.1 below
    uhat = (u0[None] * (1 - 0.5 * np.arange(Nt + 1)[:, None] / Nt)).ravel()
    return N, Nt, dt, n, LinearSource(asm, eps=1e-3), exact_velocity, u0, uhat


def test_pgd_source_control_matches_the_cpu_loop(hp, solvers):
    """pgd_source_control(increment="resolve", state_bounds=...), all-time tracking, against the CPU loop: the bars of the
    drift-control test.  Measured on the CPU: trials [5, 1, 1], smallest margin 0.36."""
    N, Nt, dt, n, ls, wind, u0, uhat = _source_case()
    tl = (Nt + 1) * n
    bounds = solvers.StateBounds(Nt, upper=0.1, gamma=1e3)
    uo, po, co, ho = sbo.pgd_source_loop(ls, u0, uhat, solvers.Observations.alltime(Nt, dt), bounds, np.zeros(tl), 1e-3,
                                         -50.0, 50.0, n, Nt, dt, 3, max_armijo=5)
    print(f"[state bounds] source PGD on the CPU: costs {ho['cost']}, trials {ho['armijo_k']}, smallest margin "
          f"{ho['armijo_margin_min']:.3e}, penalty {ho['penalty']}")
    assert ho["armijo_margin_min"] >= 1e-8
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind)
    try:
        u, p, c, h = solvers.pgd_source_control(prob, u0, uhat, np.zeros(tl), 1e-3, -50.0, 50.0, optim="alltime",
                                                increment="resolve", max_armijo=5, max_iters=3, tol=0.0,
                                                state_bounds=bounds)
    finally:
        prob.close()
    _compare_histories(h, ho, bounds.pairs(n, dt))
    print(f"[state bounds] source PGD device vs CPU: state {rel(u, uo):.2e}, control {rel(c, co):.2e}")
    assert rel(u, uo) < ADJ_TOL and rel(c, co) < ADJ_TOL and rel(p, po) < ADJ_TOL


def _history_equal(h1, h0):
    return all(h1[key] == h0[key] for key in ("cost", "armijo_k", "armijo_margin", "used", "pairs", "step"))


def test_lbfgs_solidbody(hp, solvers, pgd_case):
    """lbfgs_solidbody: inactive bounds give the history of the run without bit for bit (a context each); an active run
    has finite statistics and an accepted J + P that never increases."""
    k = pgd_case
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    od = _Order(k["mesh"], True)
    c0 = np.full((Nt + 1) * n, 0.5)

    def run(kw):
        prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
        try:
            return solvers.lbfgs_solidbody(prob, od.to_dev(k["u0"]), od.to_dev(k["tgt"][Nt * n:]), c0, k["beta"], 0.0, 5.0, 3,
                                           max_armijo=6, **kw)
        finally:
            prob.close()

    (u0_, _, c0_, h0), (u1, _, c1, h1) = run({}), run(dict(state_bounds=solvers.StateBounds(Nt, upper=50.0, gamma=10.0)))
    assert np.array_equal(u1, u0_) and np.array_equal(c1, c0_) and _history_equal(h1, h0) and h1["cost0"] == h0["cost0"]
    assert h1["penalty"] == [0.0] * len(h1["cost"])
    *_, h = run(dict(state_bounds=solvers.StateBounds(Nt, upper=0.5, gamma=200.0)))
    assert len(h["cost"]) >= 1 and len(h["penalty"]) == len(h["cost"]) == len(h["max_violation"]) == len(h["violated_fraction"])
    assert np.isfinite(h["cost"]).all() and np.isfinite(h["penalty"]).all() and np.isfinite(h["max_violation"]).all()
    assert min(h["penalty"]) > 0 and all(0 < f < 1 for f in h["violated_fraction"])
    assert np.all(np.diff([h["cost0"]] + h["cost"]) <= 0)


def test_lbfgs_source_control(hp, solvers):
    N, Nt, dt, n, ls, wind, u0, uhat = _source_case()
    tl = (Nt + 1) * n

    def run(kw):
        prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind)
        try:
            return solvers.lbfgs_source_control(prob, u0, uhat, np.zeros(tl), 1e-3, -50.0, 50.0, optim="alltime",
                                                max_armijo=5, max_iters=3, tol=0.0, **kw)
        finally:
            prob.close()

    (u0_, _, c0_, h0), (u1, _, c1, h1) = run({}), run(dict(state_bounds=solvers.StateBounds(Nt, upper=50.0, gamma=10.0)))
    assert np.array_equal(u1, u0_) and np.array_equal(c1, c0_) and _history_equal(h1, h0) and h1["cost0"] == h0["cost0"]
    assert h1["penalty"] == [0.0] * len(h1["cost"])
    *_, h = run(dict(state_bounds=solvers.StateBounds(Nt, upper=0.15, gamma=100.0)))
    assert len(h["cost"]) >= 1 and len(h["penalty"]) == len(h["cost"])
    assert np.isfinite(h["cost"]).all() and np.isfinite(h["penalty"]).all() and np.isfinite(h["max_violation"]).all()
    assert min(h["penalty"]) > 0 and all(0 < f < 1 for f in h["violated_fraction"])
    assert np.all(np.diff([h["cost0"]] + h["cost"]) <= 0)


# ------------------------------------------------------------------------------------------------ NaN, error paths, example
def test_nan_in_a_penalised_level_fails_the_solve(hp, solvers):
    """A NaN in u at a penalised level that no observation reads makes the adjoint raise NotConverged (the load is NaN:
    v is written with min / max); the context works afterwards."""
    N, Nt = 21, 6
    dt = 1e-3 * 80 / (N - 1)
    mesh, _ = _oracle(N)
    od = _Order(mesh, True)
    n, tl = mesh.nodes, (Nt + 1) * mesh.nodes
    c, u, uh = _member(mesh, Nt, dt, 0)
    obs = solvers.Observations(Nt, [2, Nt], [0.7, 1.3])
    bounds = solvers.StateBounds(Nt, lower=LO, upper=HI, gamma=GAMMA)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    ctx = prob.ctx
    try:
        dc, dh, dp = ctx.array(od.to_dev(c)), ctx.array(od.to_dev(uh)), ctx.zeros(tl)
        bad = od.to_dev(u)
        bad[4 * n + n // 2] = np.nan                            # level 4: penalised, not observed
        with pytest.raises(hp._lib.NotConverged):
            prob.adjoint(dc, ctx.array(bad), dh, dp, "snapshots", batch=1, obs=obs, state_bounds=bounds)
        prob.adjoint(dc, ctx.array(od.to_dev(u)), dh, dp.zero(), "snapshots", batch=1, obs=obs, state_bounds=bounds)
        assert rel(od.from_dev(dp.download()), _adjoint_oracle(N, Nt, dt, obs, bounds, 0)) < ADJ_TOL
    finally:
        prob.close()


def test_error_paths(hp, solvers):
    N, Nt, dt = 5, 4, 1e-3
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, solvers.finaltime_exact_wind())
    ctx, n, tl = prob.ctx, prob.n, prob.tlen
    err = hp._lib.FemFctValueError
    try:
        c, u, uh, p = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl)
        th, sg, hi = ctx.array(np.zeros(Nt + 1)), ctx.array(np.full(Nt + 1, dt)), ctx.array(np.ones(n))
        with pytest.raises(ValueError):                         # the fused linear-increment costs know two modes only
            solvers.pgd_source_control(prob, np.zeros(n), np.zeros(tl), np.zeros(tl), 1e-3, 0.0, 1.0, increment="linear",
                                       state_bounds=solvers.StateBounds(Nt, upper=1.0))
        for bad in (solvers.StateBounds(Nt, upper=np.ones(n + 1)), solvers.StateBounds(Nt + 1, upper=1.0),
                    solvers.StateBounds(Nt, upper=1.0, window=np.ones(n - 1))):
            with pytest.raises(ValueError):                     # bounds that do not fit the problem
                prob.adjoint_state(u, uh, p, "alltime", batch=1, state_bounds=bad)
            with pytest.raises(ValueError):
                prob.cost(u, uh, c, 0.1, "alltime", batch=1, state_bounds=bad)
        with pytest.raises(ValueError):
            solvers.pgd_source_control(prob, np.zeros(n), np.zeros(tl), np.zeros(tl), 1e-3, 0.0, 1.0, increment="resolve",
                                       state_bounds="upper")
        # the C entry points' argument checks
        sweep = lambda **kw: ctx.solidbody_adjoint_bounds(prob.Arot, c, u, uh, kw.get("theta", th), 1.0, None,
                                                          kw.get("lower"), kw.get("upper", hi), kw.get("gamma", 1.0),
                                                          kw.get("sigma", sg), None, p, Nt, dt)
        for kw, text in ((dict(sigma=None), "sigma is null"), (dict(upper=None), "no bound"), (dict(gamma=-1.0), "gamma"),
                         (dict(gamma=np.nan), "gamma"), (dict(theta=None), "theta is null")):
            with pytest.raises(err, match=text):
                sweep(**kw)
        with pytest.raises(err, match="sigma is null"):
            ctx.bound_load(uh, u, th, None, 1, dt, None, hi, 1.0, p)
        with pytest.raises(err, match="no bound"):
            ctx.bound_load(uh, u, th, sg, 1, dt, None, None, 1.0, p)
        with pytest.raises(err, match="g and x go together"):
            ctx.bound_load(uh, u, th, sg, 1, dt, None, hi, 1.0, p, g=u)
        with pytest.raises(err, match="gamma"):
            ctx.bound_cost(u, sg, None, hi, np.inf, Nt)
        with pytest.raises(err, match="sigma is null"):
            ctx.bound_cost(u, None, None, hi, 1.0, Nt)
        with pytest.raises(err, match="no bound"):
            ctx.linear_adjoint_react_bounds(prob.Arot, u, u, uh, th, 1.0, None, None, None, 1.0, sg, None, p, Nt, dt, 1e-3)
        sweep()                                                 # still usable
        assert ctx.bound_cost(u, sg, None, hi, 1.0, Nt)[0].tolist() == [0.0, 0.0, 0.0]
    finally:
        prob.close()


def test_example_runs_at_a_reduced_size():
    """The continuation of the example reduces the weighted violation P/gamma of the accepted iterate from the first
    stage to the last.  On the CPU loop with the example's reduced inputs (21 x 21 nodes, 20 steps, u <= 0.3, gamma = 50,
    500, 5000, three iterations each): P/gamma = 6.597e-4, 5.850e-4, 5.802e-4, last / first = 0.879, smallest Armijo
    margin 6.2e-5.  (The largest violation is no measure here: the initial Gaussian exceeds the bound, and it stays at
    0.687 in every stage.)"""
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "state_bounds_solidbody_pdeco.py"), "--reduced"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("gamma ")]
    assert len(lines) == 3 and "3 continuation stages of 3 PGD iterations" in out.stdout
    ratio = [float(ln.split("penalty/gamma =")[1].split()[0]) for ln in lines]
    print(f"[state bounds] example: P/gamma per stage {ratio}")
    assert np.isfinite(ratio).all() and ratio[-1] < ratio[0]
