"""The reaction term of the linear source-control PDECO on the device (-m gpu): solvers.LinearReactionSourceControl,
advection_FCT_PDECO_finaltime_exact.py.  The load kernel alone against the oracle's assembler, the sweeps in every kernel
regime against the CPU reference (reaction_source_oracle.py), two closed-form answers, the projected-gradient loop against
the CPU loop at the script's parameters, and the error paths."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BETA, LO, HI, EPS = 0.1, 0.0, 1.0, 1e-4
REGIME_KNOBS = ("FEMFCT_TILES", "FEMFCT_STRIPS", "FEMFCT_IMPLICIT", "FEMFCT_TILE4", "FEMFCT_T4_DPP", "FEMFCT_T4_K",
                "FEMFCT_T4_WALK", "FEMFCT_MESH_SOLVE", "FEMFCT_SINGLE_PATCH_BATCH", "FEMFCT_SPECIES_SOLVER",
                "FEMFCT_DEEP_HALO", "FEMFCT_WG_SLOTS", "FEMFCT_STRIP_K", "FEMFCT_MESH_STEP_BATCH_LARGE",
                "FEMFCT_MESH_STEP", "FEMFCT_MESH_STEP_BATCH")
NO_WIND = lambda x, y: (0.0 * x, 0.0 * y)


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


def _oracle_mesh(nc):
    """(mesh, assembler) of the oracle on the unit square, one at a time (the cases come grouped by size)"""
    if nc not in _MESH:
        from oracle.mesh import SquareMesh
        from oracle.assembly import P1Assembler
        mesh = SquareMesh(0.0, 1.0, nc)
        _MESH.clear()
        _MESH[nc] = (mesh, P1Assembler(mesh))
    return _MESH[nc]


class _Order:
    """Level-major arrays between the oracle's DoF order and the device's order (DoF order or vertex order)."""

    def __init__(self, mesh, vertex):
        self.n, self.vertex, self.v2d = mesh.nodes, vertex, mesh.vertex_to_dof

    def dev(self, a):
        a = np.asarray(a, dtype=np.float64)
        return np.ascontiguousarray(a.reshape(-1, self.n)[:, self.v2d]).ravel() if self.vertex else a.ravel().copy()

    def dof(self, a):
        if not self.vertex:
            return np.asarray(a).ravel().copy()
        out = np.empty((a.size // self.n, self.n))
        out[:, self.v2d] = a.reshape(-1, self.n)
        return out.ravel()


# ---------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("nc", [4, 45])
def test_react_load_vs_assembler(hp, nc, vertex):
    """out = M src - Mg(g) x against the oracle's assembled matrices.  5 x 5 nodes holds every node class of the
    right-diagonal mesh (both corner types, the four edges, the interior); 46 x 46 is more than one workgroup and no
    multiple of a tile width.  B = 1 and B = 3 (shared g, per-member src and x), mixed signs, and src = NULL.
    Bound: ||err|| <= 1e-12 || |M||src| + |Mg||x| || (about 40 double-precision terms per row: 1e-15 expected)."""
    mesh, asm = _oracle_mesh(nc)
    n, od = mesh.nodes, _Order(mesh, vertex)
    rng = np.random.default_rng(100 + nc)
    B = 3
    g = rng.uniform(-100.0, 40.0, n)
    src, x = rng.standard_normal((B, n)), rng.standard_normal((B, n)) * rng.uniform(0.1, 10.0, (B, 1))
    M, Mg = asm.mass(), asm.weighted_mass(lambda at: at(g))
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(0.0, 1.0, nc, hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
        gd, sd, xd, out = ctx.array(od.dev(g)), ctx.array(od.dev(src)), ctx.array(od.dev(x)), ctx.zeros(B * n)
        ctx.react_load(sd, gd, xd, out, batch=B)
        got = od.dof(out.download()).reshape(B, n)
        ctx.react_load(None, gd, xd, out, batch=B)
        got0 = od.dof(out.download()).reshape(B, n)
        worst = 0.0
        for b in range(B):
            scale = np.linalg.norm(abs(M) @ abs(src[b]) + abs(Mg) @ abs(x[b]))
            e1 = np.linalg.norm(got[b] - (M @ src[b] - Mg @ x[b])) / scale
            e0 = np.linalg.norm(got0[b] + Mg @ x[b]) / np.linalg.norm(abs(Mg) @ abs(x[b]))
            worst = max(worst, e1, e0)
            # the member alone: the same bits
            s1, x1, o1 = ctx.array(od.dev(src[b])), ctx.array(od.dev(x[b])), ctx.zeros(n)
            ctx.react_load(s1, gd, x1, o1, batch=1)
            assert od.dof(o1.download()).tobytes() == got[b].tobytes()
        print(f"[react_load] {nc + 1}^2 {'vertex' if vertex else 'fenics'}: worst scaled error {worst:.3e}")
        assert worst <= 1e-12
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- sweeps vs the CPU reference
def _sweep_data(mesh, Nt, B, seed):
    """g of the script's magnitude (-100 .. -10) varying in space and time, a sigma of both signs, per-member sources,
    initial conditions and targets (DoF order)."""
    n = mesh.nodes
    tl = (Nt + 1) * n
    rng = np.random.default_rng(seed)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    g = np.concatenate([-55.0 + 45.0 * np.sin(3 * x + 0.7 * k) * np.cos(2 * y - 0.3 * k) for k in range(Nt + 1)])
    sigma = 8.0 * np.cos(2 * np.pi * x) + 5.0 * np.cos(2 * np.pi * y)
    src = rng.standard_normal((B, tl)) * 3.0
    u0 = 1.0 + np.cos(np.pi * x) * np.cos(np.pi * y) + 0.1 * rng.random((B, n))
    uhat = 1.0 + 0.5 * rng.random((B, n))
    return g, sigma, src, u0, uhat


SWEEP_CASES = [
    pytest.param(False, 20, 1, 4, ("ROWS", "STRIPS"), id="fenics-21-B1"),
    pytest.param(True, 20, 1, 4, ("MESH",), id="vertex-21-B1"),
    pytest.param(True, 20, 8, 4, ("MESH",), id="vertex-21-B8"),
    pytest.param(True, 60, 1, 4, ("TILE32",), id="vertex-61-B1"),
    pytest.param(True, 60, 5, 4, ("TILE32",), id="vertex-61-B5"),
    pytest.param(True, 80, 14, 3, ("PATCH64",), id="vertex-81-B14"),
]


@pytest.mark.parametrize("vertex, nc, B, Nt, regimes", SWEEP_CASES)
def test_sweeps_vs_cpu_reference(hp, solvers, vertex, nc, B, Nt, regimes):
    """State, sensitivity (zero initial condition) and final-time adjoint sweeps with reaction, each compared member
    against the CPU reference (state 1e-10, adjoint 1e-9, relative l2) and against the member run alone (1e-12); the
    all-time adjoint with reaction once, at 21^2 in FEniCS order.  No step ran out of its solver budget."""
    import reaction_source_oracle as rso
    mesh, asm = _oracle_mesh(nc)
    n, od = mesh.nodes, _Order(mesh, vertex)
    tl, dt = (Nt + 1) * n, (1.0 / nc) ** 2
    g, sigma, src, u0, uhat = _sweep_data(mesh, Nt, B, 7 * nc + B)
    wind = solvers.finaltime_exact_wind()
    rs = rso.ReactionSource(asm, g, eps=EPS, wind=wind, sigma=sigma, wind_rule=rso.DEVICE_WIND_RULE)
    members = list(range(B)) if B <= 8 else [0, B // 2, B - 1]
    prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, nc), Nt, dt, wind, od.dev(g), eps=EPS,
                                               adjoint_mass=od.dev(sigma), batch=B,
                                               order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)
    ctx = prob.ctx
    no_budget = lambda b: not np.any(prob.solver_log(batch=b)["flags"] & hp.FLAG_SOLVER_BUDGET)
    try:
        if not any(k in os.environ for k in REGIME_KNOBS):
            assert ctx.kernel_regime(B) in [getattr(hp._lib, "REGIME_" + r) for r in regimes]
        ustart = np.zeros((B, tl))
        ustart[:, :n] = u0
        sd = ctx.array(np.concatenate([od.dev(s) for s in src]))
        ud = ctx.array(np.concatenate([od.dev(u) for u in ustart]))
        uhd = ctx.array(np.concatenate([od.dev(h) for h in uhat]))
        pd = ctx.zeros(B * tl)
        prob.state(sd, ud, batch=B)
        assert no_budget(B)
        prob.adjoint_state(ud, uhd, pd, "finaltime", batch=B)
        assert no_budget(B)
        ug, pg = ud.download().reshape(B, tl), pd.download().reshape(B, tl)
        errs = dict(state=0.0, adjoint=0.0, sens=0.0, state_alone=0.0, adjoint_alone=0.0)
        s1, u1, h1, p1, w1 = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(n), ctx.zeros(tl), ctx.zeros(tl)
        for b in members:
            uo = rso.forward(rs, src[b], ustart[b].copy(), n, Nt, dt)
            po = rso.adjoint(rs, uo, uhat[b], n, Nt, dt, "finaltime")
            errs["state"] = max(errs["state"], rel(od.dof(ug[b]), uo))
            # (the device adjoint starts from the device state: within the state bound of the reference's)
            errs["adjoint"] = max(errs["adjoint"], rel(od.dof(pg[b]), po))
            if B > 1:
                s1.upload(od.dev(src[b])), u1.upload(od.dev(ustart[b])), h1.upload(od.dev(uhat[b]))
                prob.state(s1, u1, batch=1)
                prob.adjoint_state(u1, h1, p1, "finaltime", batch=1)
                errs["state_alone"] = max(errs["state_alone"], rel(ug[b], u1.download()))
                errs["adjoint_alone"] = max(errs["adjoint_alone"], rel(pg[b], p1.download()))
        # sensitivity: member 0's source as the direction, level 0 zeroed by the call
        s1.upload(od.dev(src[0]))
        w1.upload(np.ones(tl))
        prob.sensitivity(s1, w1)
        assert no_budget(1)
        errs["sens"] = rel(od.dof(w1.download()), rso.forward(rs, src[0], np.zeros(tl), n, Nt, dt))
        if not vertex:      # the all-time adjoint with reaction: misfit load and reaction term in one launch
            target = 1.0 + 0.5 * np.random.default_rng(3).random(tl)
            td = ctx.array(od.dev(target))
            u1.upload(ug[0])
            prob.adjoint_state(u1, td, p1, "alltime", batch=1)
            assert no_budget(1)
            errs["adjoint_alltime"] = rel(od.dof(p1.download()), rso.adjoint(rs, od.dof(ug[0]), target, n, Nt, dt, "alltime"))
        print(f"[reaction sweeps] {nc + 1}^2 B={B}: " + ", ".join(f"{k}={v:.3e}" for k, v in errs.items()))
        assert errs["state"] <= 1e-10 and errs["sens"] <= 1e-10
        assert errs["adjoint"] <= 1e-9 and errs.get("adjoint_alltime", 0.0) <= 1e-9
        assert errs["state_alone"] <= 1e-12 and errs["adjoint_alone"] <= 1e-12
    finally:
        prob.close()


@pytest.mark.parametrize("vertex, nc", [(False, 20), (True, 20), (True, 60)], ids=["fenics-21", "vertex-21", "vertex-61"])
def test_zero_reaction_is_the_reaction_free_sweep_bitwise(hp, solvers, vertex, nc):
    """react = 0 and adjoint_mass = None: the forward and both adjoint sweeps of LinearSourceControl on the same data,
    bit for bit."""
    mesh, _ = _oracle_mesh(nc)
    n, Nt, dt = mesh.nodes, 4, (1.0 / nc) ** 2
    tl = (Nt + 1) * n
    rng = np.random.default_rng(nc)
    src, u0, uhat, target = rng.standard_normal(tl), 1.0 + rng.random(n), rng.random(n), rng.random(tl)
    order = hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS
    wind = solvers.finaltime_exact_wind()
    out = []
    for make in (lambda V: solvers.LinearSourceControl(V, Nt, dt, wind, eps=1e-3, order=order),
                 lambda V: solvers.LinearReactionSourceControl(V, Nt, dt, wind, np.zeros(tl), eps=1e-3, order=order)):
        prob = make(hp.SquareMeshP1(0.0, 1.0, nc))
        try:
            u = np.zeros(tl)
            u[:n] = u0
            prob.solve_state(src, u)
            out.append((u, prob.solve_adjoint_state(u, uhat, np.zeros(tl), "finaltime"),
                        prob.solve_adjoint_state(u, target, np.zeros(tl), "alltime")))
        finally:
            prob.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- closed-form answers
def test_known_answers_on_device(hp, solvers):
    """21 x 21, constant u0 and g = g0, no wind, eps = 0, no source: u_i = (1 - dt g0) u_{i-1}; with a constant sigma = s0
    in Aa2: p_i = (1 - dt g0) / (1 + dt s0) p_{i+1} (test_reaction_source_oracle.py derives both), to 1e-12."""
    nc, Nt, dt, g0, s0, c0 = 20, 6, 0.0025, -30.0, 4.0, 0.7
    V = hp.SquareMeshP1(0.0, 1.0, nc)
    n = V.nodes
    tl = (Nt + 1) * n
    prob = solvers.LinearReactionSourceControl(V, Nt, dt, NO_WIND, np.full(tl, g0), eps=0.0, adjoint_mass=np.full(n, s0))
    try:
        u = np.zeros(tl)
        u[:n] = c0
        prob.solve_state(np.zeros(tl), u)
        p = prob.solve_adjoint_state(np.zeros(tl), np.full(n, 1.5), np.zeros(tl), "finaltime")
    finally:
        prob.close()
    q = (1 - dt * g0) / (1 + dt * s0)
    eu = max(np.max(np.abs(u[i * n:(i + 1) * n] / (c0 * (1 - dt * g0) ** i) - 1)) for i in range(Nt + 1))
    ep = max(np.max(np.abs(p[i * n:(i + 1) * n] / (1.5 * q ** (Nt - i)) - 1)) for i in range(Nt + 1))
    print(f"[known answers] state {eu:.3e}, adjoint {ep:.3e}")
    assert eu <= 1e-12 and ep <= 1e-12


# ---------------------------------------------------------------------------------------------- the loop
_CPU_LOOP = {}


def _cpu_loop(solvers, nc, increment):
    import reaction_source_oracle as rso
    key = (nc, increment)
    if key not in _CPU_LOOP:
        pr = rso.script_problem(nc, solvers.finaltime_exact_fields, solvers.finaltime_exact_wind())
        tl = (pr["Nt"] + 1) * pr["n"]
        res = rso.pgd_source_control(rso.script_reference(pr, EPS), pr["u0"], pr["uhat_T"], np.zeros(tl), BETA, LO, HI,
                                     pr["n"], pr["Nt"], pr["dt"], g=pr["F"]["f"], optim="finaltime", increment=increment,
                                     max_iters=3, tol=0.0, stop="cost")
        _CPU_LOOP[key] = (pr, res)
    return _CPU_LOOP[key]


@pytest.mark.parametrize("increment", ["linear", "resolve"])
@pytest.mark.parametrize("nc", [10, 20])
def test_loop_matches_cpu_loop(hp, solvers, nc, increment):
    """pgd_source_control(optim="finaltime", stop="cost") on the reaction problem at the script's parameters (11 x 11 / 10
    steps, 21 x 21 / 40 steps), 3 iterations: the Armijo decisions of the CPU loop (whose margins are >= 1e-8 from their
    thresholds, test_reaction_source_oracle.py), costs to 1e-10, controls to 1e-9, state and adjoint to 1e-8, margins to
    1e-8 absolute."""
    pr, (uo, po, co, ho) = _cpu_loop(solvers, nc, increment)
    n, Nt, dt = pr["n"], pr["Nt"], pr["dt"]
    tl = (Nt + 1) * n
    prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, nc), Nt, dt, pr["wind"], pr["F"]["g"], eps=EPS,
                                               adjoint_mass=pr["sigma"])
    try:
        ug, pg, cg, hg = solvers.pgd_source_control(prob, pr["u0"], pr["uhat_T"], np.zeros(tl), BETA, LO, HI, g=pr["F"]["f"],
                                                    optim="finaltime", increment=increment, max_iters=3, tol=0.0,
                                                    stop="cost")
    finally:
        prob.close()
    dm = max(abs(a - b) for mg, mo in zip(hg["armijo_margin"], ho["armijo_margin"]) for a, b in zip(mg, mo))
    dc = max(abs(a - b) / abs(b) for key in ("cost", "cost_state") for a, b in zip(hg[key], ho[key]))
    print(f"[reaction loop] {nc + 1}^2 {increment}: armijo_k {hg['armijo_k']} (cpu {ho['armijo_k']}), cost {dc:.3e}, "
          f"control {rel(cg, co):.3e}, state {rel(ug, uo):.3e}, adjoint {rel(pg, po):.3e}, margins {dm:.3e}")
    assert hg["iterations"] == 3 == len(ho["cost"])
    assert hg["armijo_k"] == ho["armijo_k"]
    assert dc <= 1e-10
    assert rel(cg, co) <= 1e-9
    assert rel(ug, uo) <= 1e-8 and rel(pg, po) <= 1e-8
    assert [len(m) for m in hg["armijo_margin"]] == [len(m) for m in ho["armijo_margin"]] and dm <= 1e-8


# ---------------------------------------------------------------------------------------------- errors
def test_wrong_react_length_raises_before_device_work(hp, solvers, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(solvers, "Context", no_context)
    V = hp.SquareMeshP1(0.0, 1.0, 10)
    for react in (np.zeros(10 * V.nodes), np.zeros(12 * V.nodes), np.zeros(3)):
        with pytest.raises(ValueError):
            solvers.LinearReactionSourceControl(V, 10, 0.01, NO_WIND, react)
    with pytest.raises(ValueError):
        solvers.LinearReactionSourceControl(V, 10, 0.01, NO_WIND, np.zeros(11 * V.nodes), adjoint_mass=np.zeros(5))


def test_nan_in_reaction_coefficient_fails_the_sweep(hp, solvers):
    """21 x 21: one NaN in g at a level in the middle of the sweep must come out as NotConverged, not as NaN in u."""
    nc, Nt = 20, 4
    mesh, _ = _oracle_mesh(nc)
    n, dt = mesh.nodes, (1.0 / nc) ** 2
    tl = (Nt + 1) * n
    g, _, src, u0, _ = _sweep_data(mesh, Nt, 1, 11)
    g[2 * n + 57] = np.nan
    prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, nc), Nt, dt, solvers.finaltime_exact_wind(), g,
                                               eps=EPS)
    try:
        u = np.zeros(tl)
        u[:n] = u0[0]
        with pytest.raises(hp.NotConverged):
            prob.solve_state(src[0], u)
    finally:
        prob.close()
