"""Snapshot observations (``optim="snapshots"``, ``solvers.Observations``) for the nonlinear, Schnakenberg and chemotaxis
systems on the device (-m gpu), against the CPU reference tests/systems_snapshots_oracle.py, in every kernel regime.
Set-up, tolerances and the log checks are those of tests/test_gpu_systems_regimes.py (its helpers are used as they are):
per-member random data as in tests/test_gpu_chtxs_growth.py, dt = 5e-4, 6 steps; adjoints to 1e-9, a member against itself
run alone to 1e-12; no solve out of budget, residuals <= 1e-13.  u is observed at levels [2, 5] with weights (1, 0.5), v at
[3, 6]: one terminal level observed, one not.  Unobserved target levels hold NaN in every case.

PGD test: the CPU loop accepts the chemotaxis driver's first trial step s0 = 2 (and 0.8, 0.3, 0.1) at once; with s0 = 4 it
rejects once and then accepts in both iterations.  Its Armijo margins (> 0: rejected): 5.15e-3, -0.487; 0.931, -0.408 -- all
far above 1e-6 in size.  (s0 = 3: 1.49e-3, -0.908; 1.78, -0.819.  s0 = 6: three trials per iteration.)"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import systems_snapshots_oracle as sso
import chtxs_growth_oracle as go
import test_gpu_systems_regimes as reg

pytestmark = pytest.mark.gpu

MIMURA = (0.0, 1.0, -1.0)
ADJ_TOL = reg.ADJ_TOL
DT, NT = 5e-4, 6
LEVELS_U, WEIGHTS_U, LEVELS_V = [2, 5], [1.0, 0.5], [3, 6]
rel = reg.rel

PGD_S0 = 4.0
PGD_OPTS = dict(max_iter_GD=2, max_iter_armijo=6, tol=0.0, s0=PGD_S0)

# nodes per side, batch, DoF order, regimes (the smallest sizes that reach each, from tests/test_gpu_chtxs_growth.py's CASES)
# and what the case adds: "window" (zero on half of the domain), "u-only" (obs = (obs_u, None), no v target), "wind"
# (Schnakenberg's time-dependent wind), "growth" (chemotaxis with (0, 1, -1))
R21 = (21, 1, "fenics", ("ROWS", "STRIPS"))
R41, R41B = (41, 1, "vertex", ("MESH",)), (41, 8, "vertex", ("MESH",))
R46, R47B, R81B = (46, 1, "vertex", ("TILE32",)), (47, 8, "vertex", ("TILE32",)), (81, 14, "vertex", ("PATCH64",))
CASES = [
    pytest.param("nonlinear", *R21, (), id="nonlinear-N21-B1-fenics-order"),
    pytest.param("nonlinear", *R41B, (), id="nonlinear-N41-B8-one-workgroup"),
    pytest.param("nonlinear", *R46, ("window",), id="nonlinear-N46-B1-tile32-window"),
    pytest.param("nonlinear", *R81B, (), id="nonlinear-N81-B14-patch64"),
    pytest.param("schnak", *R21, (), id="schnak-N21-B1-fenics-order"),
    pytest.param("schnak", *R41B, ("wind", "u-only"), id="schnak-N41-B8-one-workgroup-wind-u-only"),
    pytest.param("schnak", *R46, ("window",), id="schnak-N46-B1-tile32-window"),
    pytest.param("schnak", *R81B, (), id="schnak-N81-B14-patch64"),
    pytest.param("chtxs", *R21, ("window",), id="chtxs-N21-B1-fenics-order-window"),
    pytest.param("chtxs", *R41, ("u-only",), id="chtxs-N41-B1-one-workgroup-u-only"),
    pytest.param("chtxs", *R41B, ("growth",), id="chtxs-N41-B8-one-workgroup-growth"),
    pytest.param("chtxs", *R46, ("window", "growth"), id="chtxs-N46-B1-tile32-window-growth"),
    pytest.param("chtxs", *R47B, (), id="chtxs-N47-B8-single-patch"),
    pytest.param("chtxs", *R81B, ("growth",), id="chtxs-N81-B14-patch64-growth"),
]


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def systems():
    return importlib.import_module("fem-fct-pdeco_amd.systems")


@pytest.fixture(scope="module")
def Observations():
    return importlib.import_module("fem-fct-pdeco_amd.solvers").Observations


@pytest.fixture(scope="module")
def DeviceObs():
    return importlib.import_module("fem-fct-pdeco_amd.device").DeviceObs


def _members(system, N, B, order):
    mem = reg._Members(system, N, B, NT)
    if order == "fenics":                      # the device works in DoF order: nothing to permute
        mem.v2d = np.arange(mem.n)
    return mem


def _only(a, levels, n):
    """the trajectories ``a`` (B x tl) with NaN at every level but ``levels``"""
    out = np.full_like(a, np.nan)
    for lv in levels:
        out[:, lv * n:(lv + 1) * n] = a[:, lv * n:(lv + 1) * n]
    return out


def _s(t):                                                         # separable wind s(t) w0(x)
    return 1.5 * np.cos(40.0 * t) - 0.25


class _Problem:
    """One system on one context: its forward sweep (per-step control), the three adjoint sweeps as
    ``sweep(u, [v,] uhat, [vhat,] [c,] p, [q,] batch)`` closures, and the CPU reference of the snapshot adjoint."""

    def __init__(self, hp, systems, S, system, flags=()):
        self.S, self.ctx, self.system, self.two = S, S.ctx, system, system != "nonlinear"
        self.growth = MIMURA if "growth" in flags else None
        self.wind = "wind" in flags
        if system == "nonlinear":
            self.eps, _, wind = systems.get_nonlinear_eqns_params()
            self.Aw, _ = S.convection(wind, "nonlinear")
        elif system == "schnak":
            self.par, wind = systems._schnak_par()
            self.Aw, self.AwT = S.convection(wind, "schnak")
            self.ws = systems._wind_factors(_s, NT, DT) if self.wind else None
            self.ws_adj = systems._wind_factors(_s, NT, DT, T=NT * DT) if self.wind else None
        else:
            self.cpar = systems._chtxs_par()

    def initial(self, mem):
        n, x, y = mem.n, mem.x, mem.y
        if self.system == "nonlinear":
            return [[5 * y * (y - 1) * x * (x - 1) * np.sin(4 * np.pi * x) + 0.05 * r.random(n) for r in mem.rngs]], \
                np.stack([r.random(mem.tl) for r in mem.rngs])
        if self.system == "schnak":
            return [[1.0 + 0.1 * np.cos(2 * np.pi * (x + y)) + 0.02 * r.random(n) for r in mem.rngs],
                    [0.9 + 0.1 * np.cos(2 * np.pi * (x - y)) + 0.02 * r.random(n) for r in mem.rngs]], \
                np.stack([0.1 + 0.05 * r.random(mem.tl) for r in mem.rngs])
        return [[1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs], [1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs]], \
            np.stack([20 * r.random(mem.tl) for r in mem.rngs])

    def forward(self, c_, *uv_b):
        ctx, b = self.ctx, uv_b[-1]
        if self.system == "nonlinear":
            ctx.nonlinear_forward_ct(self.Aw, c_, uv_b[0], NT, DT, self.eps, batch=b)
        elif self.system == "schnak":
            ctx.schnak_forward_ct(self.Aw, c_, uv_b[0], uv_b[1], NT, DT, self.par, 1.0, batch=b, wind_scale=self.ws)
        else:
            ctx.chtxs_forward_ct(c_, uv_b[0], uv_b[1], NT, DT, self.cpar, 0.1, batch=b, growth=self.growth)

    def adjoint(self, alltime=False, obs=None, misfit="mass", v_target=True):
        """the sweep closure for reg._Device.run: inputs (u, [v,] uhat, [vhat,] [c]), outputs (p, [q]), batch"""
        ctx = self.ctx
        if self.system == "nonlinear":
            return lambda u_, t_, p_, b: ctx.nonlinear_adjoint(self.Aw, u_, t_, p_, NT, DT, self.eps, batch=b, alltime=alltime, obs=obs)
        if self.system == "schnak":
            f = lambda u_, v_, tu, tv, p_, q_, b: ctx.schnak_adjoint(self.AwT, u_, v_, tu, tv, p_, q_, NT, DT, self.par, batch=b,
                                                                     alltime=alltime, wind_scale=self.ws_adj, obs=obs)
            return f if v_target else (lambda u_, v_, tu, p_, q_, b: f(u_, v_, tu, None, p_, q_, b))
        f = lambda u_, v_, tu, tv, c_, p_, q_, b: ctx.chtxs_adjoint(u_, v_, tu, tv, p_, q_, c_, NT, DT, self.cpar, 0.1,
                                                                    alltime=alltime, batch=b, growth=self.growth, obs=obs,
                                                                    misfit=misfit)
        return f if v_target else (lambda u_, v_, tu, c_, p_, q_, b: f(u_, v_, tu, None, c_, p_, q_, b))

    def reference(self, asm, mem, m, st, hats, c, obs, misfit="mass"):
        """the CPU snapshot adjoint of member m (DoF order): [p] or [p, q]"""
        n, tl, d = mem.n, mem.tl, mem.to_dof
        hat = [None if h is None else d(h[m]) for h in hats]
        if self.system == "nonlinear":
            return [sso.solve_adjoint_nonlinear_equation(d(st[0][m]), hat[0], np.zeros(tl), NT * DT, asm, n, NT, DT, obs)]
        if self.system == "schnak":
            return list(sso.solve_adjoint_schnak_system(d(st[0][m]), d(st[1][m]), hat[0], hat[1], np.zeros(tl), np.zeros(tl),
                                                        NT * DT, asm, n, NT, DT, obs, wind_scale=_s if self.wind else None))
        return list(sso.solve_adjoint_chtxs_system(d(st[0][m]), d(st[1][m]), hat[0], hat[1], np.zeros(tl), np.zeros(tl), d(c[m]),
                                                   NT * DT, asm, n, NT, DT, obs, misfit=misfit, growth=self.growth))


def _device_obs(ctx, DeviceObs, ou, ov, window):
    """the observations on the device (window: device order) and the arrays to free"""
    arrays = [ctx.array(o.theta) for o in (ou, ov) if o is not None]
    th = iter(arrays)
    dev = DeviceObs(theta_u=next(th) if ou is not None else None, tau_u=0.0 if ou is None else ou.tau,
                    theta_v=next(th) if ov is not None else None, tau_v=0.0 if ov is None else ov.tau,
                    window=None if window is None else ctx.array(window))
    return dev, arrays + ([dev.window] if window is not None else [])


def _states_and_targets(P, D, mem):
    """device forward sweep of every member, then targets next to the states (test_gpu_chtxs_growth.py's recipe)"""
    x0, c = P.initial(mem)
    st = D.run(P.forward, [mem.traj(a) for a in x0], [c], mem.B)
    fac = (0.8, 0.05) if P.system == "nonlinear" else (0.9, 0.02)
    hats = [np.stack([fac[0] * st[0][m] + fac[1] * r.random(mem.tl) for m, r in enumerate(mem.rngs)])]
    if P.two:
        hats.append(np.stack([(1.1 if P.system == "schnak" else 1.05) * st[1][m] + 0.02 * r.random(mem.tl)
                              for m, r in enumerate(mem.rngs)]))
    return st, hats, c


@pytest.mark.parametrize("system, N, B, order, regimes, flags", CASES)
def test_snapshot_adjoint_vs_reference(hp, systems, Observations, DeviceObs, system, N, B, order, regimes, flags):
    """The snapshot adjoint of ``system`` on B members in the kernel regime the case names: each member against the CPU
    reference (1e-9) and against itself run alone (1e-12), solver logs clean, NaN at every unobserved target level, and the
    answer more than 1e-4 (relative l2) away from the all-time and the final-time sweeps of the same data, so that an
    ignored keyword cannot pass.  Chemotaxis runs both loads."""
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    S = systems.PDESystems(V, order=hp.ORDER_FENICS if order == "fenics" else hp.ORDER_VERTEX)
    arrays = []
    try:
        knobs = reg._regime_knobs_default()
        if knobs:
            assert S.ctx.kernel_regime(B) in [getattr(hp._lib, "REGIME_" + r) for r in regimes]
        _, asm = reg._oracle(N)
        mem = _members(system, N, B, order)
        n, tl = mem.n, mem.tl
        assert n == S.ctx.n == N * N
        P = _Problem(hp, systems, S, system, flags)
        D = reg._Device(hp, S.ctx, NT, species=P.two, cheb=knobs and order == "vertex")
        st, hats, c = _states_and_targets(P, D, mem)
        mesh = reg._oracle(N)[0]
        x_dev = mem.x if order == "vertex" else mesh.x[mesh.dof_to_vertex]               # coordinates in the device's order
        window = np.where(x_dev > 0.5, 1.0, 0.0) if "window" in flags else None
        w_dof = None if window is None else mem.to_dof(window)
        ou = Observations(NT, LEVELS_U, WEIGHTS_U, window=w_dof)
        ov = Observations(NT, LEVELS_V, window=w_dof) if P.two and "u-only" not in flags else None
        obs_ref = ou if not P.two else (ou, ov)
        dev, arrays = _device_obs(S.ctx, DeviceObs, ou, ov, window)
        tg = [_only(hats[0], LEVELS_U, n)] + ([_only(hats[1], LEVELS_V, n)] if ov is not None else [])
        tg_ref = tg + ([None] if P.two and ov is None else [])
        ins = st + tg + ([c] if system == "chtxs" else [])
        zeros = [np.zeros((B, tl)) for _ in range(2 if P.two else 1)]
        errs = {}
        got = {}
        for misfit in (("mass", "nodal") if system == "chtxs" else ("mass",)):
            got[misfit] = reg._compare(f"pq_{misfit}", D, mem, P.adjoint(obs=dev, misfit=misfit, v_target=ov is not None), zeros,
                                       ins, lambda m, mf=misfit: P.reference(asm, mem, m, st, tg_ref, c, obs_ref, mf), ADJ_TOL, errs)
            assert all(np.isfinite(g).all() for g in got[misfit])
        if system == "chtxs":
            errs["nodal_vs_mass"] = rel(got["nodal"][0], got["mass"][0])
            assert errs["nodal_vs_mass"] > 1e-4, errs
        full = st + hats + ([c] if system == "chtxs" else [])
        fin = st + [h[:, NT * n:] for h in hats] + ([c] if system == "chtxs" else [])
        p_all = D.run(P.adjoint(alltime=True), zeros, full, B)[0]
        p_fin = D.run(P.adjoint(alltime=False), zeros, fin, B)[0]
        errs["vs_alltime"], errs["vs_finaltime"] = rel(got["mass"][0], p_all), rel(got["mass"][0], p_fin)
        reg._report(f"snapshots {system} N={N} B={B} {order} {'/'.join(regimes)} {'+'.join(flags)}", **errs)
        assert errs["vs_alltime"] > 1e-4 and errs["vs_finaltime"] > 1e-4, errs
        if "window" in flags:                   # the terminal condition vanishes where the window does
            assert not got["mass"][0][:, NT * n:][:, window == 0.0].any()
    finally:
        for a in arrays:
            a.free()
        S.close()


@pytest.mark.parametrize("N, order", [(21, "fenics"), (46, "vertex")])
@pytest.mark.parametrize("system", ["nonlinear", "schnak", "chtxs", "chtxs-growth", "schnak-wind"])
def test_corners_equal_the_existing_sweeps_bit_for_bit(hp, systems, Observations, DeviceObs, system, N, order):
    """Observations.finaltime(Nt) and Observations.alltime(Nt, dt) without a window (chemotaxis: misfit="nodal") give the
    bits of the existing final-time and all-time entry points.  Each sweep on a fresh context: a context's second sweep of
    a kind runs with the budgets its first one settled, which decide a tile step's bits."""
    flags = tuple(f for f in ("growth", "wind") if system.endswith(f))
    sysname = system.split("-")[0]
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)

    def fresh(run):
        S = systems.PDESystems(V, order=hp.ORDER_FENICS if order == "fenics" else hp.ORDER_VERTEX)
        arrays = []
        try:
            mem = _members(sysname, N, 1, order)
            P = _Problem(hp, systems, S, sysname, flags)
            D = reg._Device(hp, S.ctx, NT, species=P.two, cheb=False)
            st, hats, c = _states_and_targets(P, D, mem)
            return run(S, P, D, mem, st, hats, c, arrays)
        finally:
            for a in arrays:
                a.free()
            S.close()

    def existing(alltime):
        def run(S, P, D, mem, st, hats, c, arrays):
            tg = hats if alltime else [h[:, NT * mem.n:] for h in hats]
            return D.run(P.adjoint(alltime=alltime), [np.zeros((1, mem.tl)) for _ in st], st + tg + ([c] if sysname == "chtxs" else []), 1)
        return run

    def snapshots(alltime):
        def run(S, P, D, mem, st, hats, c, arrays):
            o = Observations.alltime(NT, DT) if alltime else Observations.finaltime(NT)
            dev, arr = _device_obs(S.ctx, DeviceObs, o, o if P.two else None, None)
            arrays += arr
            tg = hats if alltime else [_only(h, [NT], mem.n) for h in hats]
            return D.run(P.adjoint(obs=dev, misfit="nodal"), [np.zeros((1, mem.tl)) for _ in st],
                         st + tg + ([c] if sysname == "chtxs" else []), 1)
        return run

    for alltime in (False, True):
        old, new = fresh(existing(alltime)), fresh(snapshots(alltime))
        for a, b in zip(old, new):
            assert np.abs(a[:, :NT * N * N]).max() > 0
            assert np.array_equal(a, b), (system, N, alltime, rel(b, a))


@pytest.mark.parametrize("system", ["nonlinear", "schnak", "chtxs"])
def test_replayed_graph_reads_the_new_weights(hp, systems, Observations, DeviceObs, system):
    """theta is read on the device: observations changed in place (same device pointers, so the same captured graph)
    between two sweeps on one context give the second observations' answer."""
    N = 41
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
    arrays = []
    try:
        _, asm = reg._oracle(N)
        mem = _members(system, N, 1, "vertex")
        n, tl = mem.n, mem.tl
        P = _Problem(hp, systems, S, system)
        D = reg._Device(hp, S.ctx, NT, species=P.two, cheb=reg._regime_knobs_default())
        st, hats, c = _states_and_targets(P, D, mem)
        first = (Observations(NT, LEVELS_U, WEIGHTS_U), Observations(NT, [3, 5]))
        second = (Observations(NT, [1, 5], [2.0, 0.25]), Observations(NT, [3, 5], [0.5, 3.0]))
        dev, arrays = _device_obs(S.ctx, DeviceObs, first[0], first[1] if P.two else None, None)
        d_in = [S.ctx.array(np.ascontiguousarray(a).ravel()) for a in st + hats + ([c] if system == "chtxs" else [])]
        d_out = [S.ctx.zeros(tl) for _ in st]
        arrays += d_in + d_out
        sweep = P.adjoint(obs=dev)
        sweep(*d_in, *d_out, 1)
        sweep(*d_in, *d_out, 1)                 # budgets settled: the graph the third sweep replays
        before = [d.download() for d in d_out]
        dev.theta_u.upload(second[0].theta)
        if P.two:
            dev.theta_v.upload(second[1].theta)
        sweep(*d_in, *d_out, 1)
        after = [d.download() for d in d_out]
        ref = P.reference(asm, mem, 0, [s for s in st], hats, c, second[0] if not P.two else second)
        errs = {f"x{k}": rel(mem.to_dof(a), r) for k, (a, r) in enumerate(zip(after, ref))}
        errs["moved"] = rel(after[0], before[0])
        reg._report(f"snapshots {system} theta changed in place N={N}", **errs)
        assert errs["moved"] > 1e-4 and max(v for k, v in errs.items() if k != "moved") < ADJ_TOL, errs
    finally:
        for a in arrays:
            a.free()
        S.close()


def test_form_groups_off_gives_the_same_bits(hp, systems, Observations, DeviceObs, monkeypatch):
    """FEMFCT_FORM_GROUPS=0 (every form in its own launch) gives the bits of the grouped launches, chemotaxis with growth
    and a window, both loads; each on a fresh context."""
    N = 41
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    out = []
    for groups in ("1", "0"):
        monkeypatch.setenv("FEMFCT_FORM_GROUPS", groups)
        S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
        arrays = []
        try:
            mem = _members("chtxs", N, 1, "vertex")
            P = _Problem(hp, systems, S, "chtxs", ("growth",))
            D = reg._Device(hp, S.ctx, NT, species=True, cheb=False)
            st, hats, c = _states_and_targets(P, D, mem)
            window = np.where(mem.x > 0.5, 1.0, 0.0)
            w_dof = mem.to_dof(window)
            dev, arrays = _device_obs(S.ctx, DeviceObs, Observations(NT, LEVELS_U, WEIGHTS_U, window=w_dof),
                                      Observations(NT, LEVELS_V, window=w_dof), window)
            zeros = [np.zeros((1, mem.tl)), np.zeros((1, mem.tl))]
            out.append([D.run(P.adjoint(obs=dev, misfit=mf), zeros, st + hats + [c], 1) for mf in ("mass", "nodal")])
        finally:
            for a in arrays:
                a.free()
            S.close()
    for a, b in zip(out[0], out[1]):
        for x, y in zip(a, b):
            assert np.abs(x).max() > 0 and np.array_equal(x, y)


def test_cost_of_two_variables(hp, Observations):
    """SystemPDECO._cost with optim="snapshots" (femfct_obs_cost per state variable plus the control term) against the CPU
    cost to 1e-12 relative, and the same bits at B = 1 and as every member of B = 8."""
    N, Nt = 41, NT
    mesh, asm = reg._oracle(N)
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    n = V.nodes
    tl = (Nt + 1) * n
    rng = np.random.default_rng(7)
    x = mesh.x[mesh.dof_to_vertex]
    w = np.where(x > 0.5, 1.0, 0.25)
    obs = (Observations(Nt, LEVELS_U, WEIGHTS_U, window=w), Observations(Nt, LEVELS_V, window=w))
    u, v, c = 1.5 + 0.1 * rng.random(tl), 1.2 + 0.1 * rng.random(tl), 20 * rng.random(tl)
    uhat, vhat = 0.9 * u + 0.02 * rng.random(tl), 1.05 * v + 0.02 * rng.random(tl)
    only = lambda a, lv: _only(a[None], lv, n)[0]
    uhat, vhat = only(uhat, LEVELS_U), only(vhat, LEVELS_V)
    J_ref = sso.cost(asm, asm.mass(), u, uhat, v, vhat, c, obs, n, Nt, DT, 1e-3)
    with hp.SystemPDECO("chtxs", V, Nt, DT, optim="snapshots", obs=obs, growth=MIMURA, control_per_step=True) as prob:
        rep = lambda a, B: prob._up(np.tile(a, B))
        J1 = prob._cost(rep(u, 1), rep(v, 1), rep(c, 1), [rep(uhat, 1), rep(vhat, 1)], 1)
        J8 = prob._cost(rep(u, 8), rep(v, 8), rep(c, 8), [rep(uhat, 8), rep(vhat, 8)], 8)
    print(f"[regimes] snapshots cost: device {J1[0]:.17g}, reference {J_ref:.17g}, rel {abs(J1[0] - J_ref) / abs(J_ref):.2e}")
    assert J1.shape == (1,) and J8.shape == (8,) and np.isfinite(J1).all()
    assert abs(J1[0] - J_ref) <= 1e-12 * abs(J_ref)
    assert np.all(J8 == J1[0])


@pytest.mark.parametrize("speculative", [True, False], ids=["speculative", "sequential"])
def test_pgd_with_snapshots_vs_reference(hp, Observations, speculative):
    """SystemPDECO("chtxs", optim="snapshots", growth=(0, 1, -1), control_per_step=True) at 41 x 41, 10 steps, both variables
    observed at levels {4, 10}, two iterations, against the CPU loop (systems_snapshots_oracle.chtxs_pgd_loop): the same
    Armijo trial counts, costs to 1e-9, final c, u, v, p, q to 1e-7 (the bounds of the existing PGD tests).  The reference
    loop both rejects and accepts, with every Armijo margin at least 1e-6 in size (see the header)."""
    N, Nt, dt = 41, 10, 5e-4
    mesh, asm = reg._oracle(N)
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    n = V.nodes
    tl = (Nt + 1) * n
    z = lambda x0: np.concatenate([x0, np.zeros(Nt * n)])
    rng = np.random.default_rng(41)
    u0 = 1.5 + 0.1 * (0.5 - rng.random(n))
    v0 = u0.copy()
    obs = Observations(Nt, [4, 10])

    def reference():
        ut, vt = go.solve_chtxs_system(np.full(tl, 10.0), z(u0), z(v0), asm, n, Nt, dt, growth=MIMURA, per_step=True)
        targets = tuple(_only(a[None], [4, 10], n)[0] for a in (ut, vt))
        return targets, sso.chtxs_pgd_loop(asm, asm.mass(), (u0, v0), targets, obs, Nt, dt, MIMURA, s0=PGD_S0,
                                           max_iter_armijo=PGD_OPTS["max_iter_armijo"], iters=2)
    targets, ref = reg._cached(("chtxs_snapshots_pgd", N), reference)
    mref = [m for ms in ref["armijo_margin"] for m in ms]
    assert max(ref["armijo_its"]) >= 2 and max(ref["armijo_its"]) < PGD_OPTS["max_iter_armijo"]    # rejects, then accepts
    assert min(abs(m) for m in mref) >= 1e-6, mref
    got = hp.projected_gradient_descent("chtxs", V, (u0, v0), targets, Nt, dt, speculative=speculative, control_per_step=True,
                                        growth=MIMURA, optim="snapshots", obs=obs, **PGD_OPTS)
    errs = {k: rel(got[k], ref[k]) for k in ("c", "u", "v", "p", "q")}
    reg._report(f"chtxs snapshots PGD 41^2 x {Nt} steps, {'speculative' if speculative else 'sequential'}: armijo_its "
                f"{got['armijo_its']}, margins {['%.3g' % m for m in mref]}", **errs)
    assert got["it"] == 2 and not got["restored"]
    assert got["armijo_its"] == ref["armijo_its"], (got["armijo_its"], ref["armijo_its"])
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9)
    assert max(errs.values()) < 1e-7, errs


def test_invalid_arguments(hp, systems, Observations, DeviceObs):
    N, Nt = 21, 4
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    n = V.nodes
    tl = (Nt + 1) * n
    ok = Observations(Nt, [2, 4])
    z = lambda: np.zeros(tl)
    u = np.full(tl, 1.5)
    bad_obs = [None, Observations(Nt + 1, [2]), Observations(Nt, [2], window=np.ones(n - 1)), (ok, ok, ok), (None, None),
               (ok, Observations(Nt, [2], window=np.ones(n)))]
    for obs in bad_obs:
        with pytest.raises(ValueError):
            hp.SystemPDECO("chtxs", V, Nt, DT, optim="snapshots", obs=obs)
        with pytest.raises(ValueError):
            systems.solve_adjoint_chtxs_system(u, u, u, u, z(), z(), u, Nt * DT, V, n, Nt, DT, None, "snapshots", obs=obs)
        with pytest.raises(ValueError):
            systems.solve_adjoint_schnak_system(u, u, u, u, z(), z(), Nt * DT, V, n, Nt, DT, None, optim="snapshots", obs=obs)
    for obs in (None, (ok, ok), (ok, None), Observations(Nt + 1, [2])):     # a pair for the one-variable problem
        with pytest.raises(ValueError):
            hp.SystemPDECO("nonlinear", V, Nt, DT, optim="snapshots", obs=obs)
        with pytest.raises(ValueError):
            systems.solve_adjoint_nonlinear_equation(u, u, z(), Nt * DT, V, n, Nt, DT, None, optim="snapshots", obs=obs)
    with pytest.raises(ValueError):
        hp.SystemPDECO("chtxs", V, Nt, DT, optim="snapshots", obs=ok, misfit="lumped")
    with pytest.raises(ValueError):
        hp.SystemPDECO("schnak", V, Nt, DT, optim="snapshots", obs=ok, misfit="nodal")
    with pytest.raises(ValueError):
        hp.SystemPDECO("chtxs", V, Nt, DT, optim="alltime", obs=ok)
    with pytest.raises(ValueError, match="Must be one of"):
        hp.SystemPDECO("chtxs", V, Nt, DT, optim="sometimes")
    with pytest.raises(ValueError):                                         # a target of the wrong size
        systems.solve_adjoint_chtxs_system(u, u, u[:n], u, z(), z(), u, Nt * DT, V, n, Nt, DT, None, "snapshots", obs=ok)
    with pytest.raises(ValueError):
        with hp.SystemPDECO("chtxs", V, Nt, DT, optim="snapshots", obs=ok) as prob:
            prob.run((u[:n], u[:n]), (u[:n], u[:n]))
    S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
    try:
        ctx = S.ctx
        d = ctx.array(u)
        th = ctx.array(ok.theta)
        p, q = ctx.zeros(tl), ctx.zeros(tl)
        cpar = systems._chtxs_par()
        for tau in (np.nan, np.inf):
            with pytest.raises(ValueError):
                ctx.chtxs_adjoint(d, d, d, d, p, q, d, Nt, DT, cpar, 0.1, obs=DeviceObs(th, tau, th, 0.0))
        with pytest.raises(ValueError):
            ctx.chtxs_adjoint(d, d, d, d, p, q, d, Nt, DT, cpar, 0.1, obs=DeviceObs(th, 1.0, th, 1.0), misfit="lumped")
        with pytest.raises(ValueError):                                     # u observed without its target
            ctx.chtxs_adjoint(d, d, None, d, p, q, d, Nt, DT, cpar, 0.1, obs=DeviceObs(th, 1.0, th, 1.0))
        ctx.chtxs_adjoint(d, d, d, None, p, q, d, Nt, DT, cpar, 0.1, obs=DeviceObs(th, 1.0, None, 0.0))    # v not observed
        assert np.isfinite(p.download()).all() and not q.download()[Nt * n:].any()
    finally:
        S.close()


def test_example_runs_in_its_reduced_mode():
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "chemotaxis_mimura_snapshots_pdeco.py"), "--reduced", "--iters", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "33 x 33" in out.stdout and "levels [3, 6]" in out.stdout and out.stdout.count("cost ") >= 3, out.stdout
