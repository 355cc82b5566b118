"""Every trajectory sweep across captured-graph boundaries (-m gpu).

A sweep is enqueued as graphs of FEMFCT_STEPS_PER_GRAPH time steps (default 50): a production sweep replays one graph at
successive starting levels and finishes with a shorter one, the sweeps of the other test files are one graph launched
once.  Here every sweep of tests/graph_chunks_cases.py (all 26 ``femfct_*_(forward|adjoint)*`` entry points in their
modes), 7 steps, runs on the same inputs

    eager       graphs off, one step per group: every step its own enqueue, the counters move every step   (the reference)
    one-graph   FEMFCT_STEPS_PER_GRAPH=50: 7 steps in one graph (what the rest of the suite runs)
    3+3+1       =3: the 3-step graph replayed at another level, then a one-step tail
    4+3         =4: two different multi-step graphs, none replayed
    7x1         =1: one graph replayed seven times
    profiling   per-class profiling: no graphs and no fused step end

each on a fresh context (the knob is read in femfct_create), each sweep twice (the second at the settled budget), and
must give the reference's bits: every output trajectory, every field of the step log and, for the systems with a species
solve, of its log.  The kernel regimes differ in where the step end and the level reads live; REGIMES has the smallest
mesh that reaches each.  Bitwise equality is what the project claims for graphs on and off
(test_gpu_traj.py::test_graph_relative_levels_match_eager_stepping), not a measurement.

The two anchors at the end run 53 steps with the knob at its default (graphs of 50 + 3 steps) against the CPU oracle and
print their errors beside those of the same sweep as one graph (FEMFCT_STEPS_PER_GRAPH=64); the errors measured on an
MI355X are in DESIGN.md ("A sweep does not depend on how it is cut into graphs")."""
import ctypes
import importlib

import numpy as np
import pytest

import chtxs_growth_oracle as go
import graph_chunks_cases as gc
import state_bounds_oracle as sbo
import systems_snapshots_oracle as sso
from graph_chunks_cases import NT
from regime_helpers import regime_knobs_default

pytestmark = pytest.mark.gpu

STATE_TOL, ADJ_TOL = 1e-10, 1e-9        # tests/test_gpu_systems_regimes.py, tests/test_gpu_snapshots.py

# name -> (graphs, FEMFCT_STEPS_PER_GRAPH or None for the default, profiling); the first one is the reference
VARIANTS = {"eager": (False, "1", False), "one-graph": (True, "50", False), "3+3+1": (True, "3", False),
            "4+3": (True, "4", False), "7x1": (True, "1", False), "profiling": (True, None, True)}

# nodes per side, DoF order, batch, the regime femfct_kernel_regime reports, the cases (None: all), the species solver
REGIMES = {
    "mesh-B1": (21, "vertex", 1, ("MESH",), None, "auto"),          # k_mesh_step, one-workgroup species solve, fused end
    "mesh-B3": (21, "vertex", 3, ("MESH",), None, "auto"),
    "tile32-B1": (46, "vertex", 1, ("TILE32",), None, "auto"),      # tile kernels, tile Chebyshev species solve
    "rows-B2": (21, "fenics", 2, ("ROWS", "STRIPS"), None, "auto"),     # row kernels, the k_step_end launch
    "patch64-B14": (81, "vertex", 14, ("PATCH64",), ("sb-fwd-src-eps0", "sb-adj-bounds"), "auto"),
    "bicgstab-B1": (21, "vertex", 1, ("MESH",), ("sk-fwd", "sk-adj-alltime"), "bicgstab"),      # the k_kry_finish log path
}
PARAMS = [pytest.param(rid, c.id, id=f"{rid}-{c.id}") for rid, r in REGIMES.items() for c in gc.CASES
          if r[4] is None or c.id in r[4]]


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def systems():
    return importlib.import_module("fem-fct-pdeco_amd.systems")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _host(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)


class _Run:
    """One sweep of a case on a fresh context: uploads the inputs in the context's DoF order, runs the sweep twice,
    returns the outputs and the logs."""

    def __init__(self, hp, systems, case, N, order, B, species_solver):
        self.hp, self.case, self.B, self.N = hp, case, B, N
        self.dev = importlib.import_module("fem-fct-pdeco_amd.device")
        a1, a2 = gc.DOMAIN[case.family]
        V = hp.SquareMeshP1(a1, a2, N - 1)
        self.v2d = V.vertex_to_dof if order == "fenics" else None
        self.S = systems.PDESystems(V, order=hp.ORDER_FENICS if order == "fenics" else hp.ORDER_VERTEX)
        self.ctx, self.n = self.S.ctx, self.S.n
        self.systems = systems
        if species_solver != "auto":
            self.ctx.set_species_solver(species_solver)

    def close(self):
        self.S.close()

    # -- uploads
    def up(self, a):
        """host array (..., n) in vertex order -> device array in the context's order"""
        a = np.asarray(a, dtype=np.float64)
        if self.v2d is not None and a.shape[-1] == self.n:
            o = np.empty_like(a)
            o[..., self.v2d] = a
            a = o
        return self.ctx.array(np.ascontiguousarray(a).ravel())

    def traj0(self, x0):
        """B trajectories of zeros with level 0 set"""
        a = np.zeros((self.B, NT + 1, self.n))
        a[:, 0] = x0
        return self.up(a)

    def zeros(self):
        return self.ctx.zeros(self.B * (NT + 1) * self.n)

    def opt(self, d, name):
        return self.up(d[name]) if name in d else None

    # -- the families
    def sweep(self, d):
        """-> (callable that enqueues the sweep, list of the output device arrays)"""
        return getattr(self, "_" + self.case.family)(d)

    def _solidbody(self, d, linear=False):
        ctx, o, B, dt, lib, dptr = self.ctx, self.case.opts, self.B, d["dt"], self.hp._lib, self.dev.dptr
        if linear:
            wind = lambda x, y: gc.linear_wind(x, y)
            A, _ = self.S.convection(wind, "linear")
            eps, drift, c, c_shared = (1e-4 if o.get("g") else 1e-3), (0.0, 0.0), ctx.zeros((NT + 1) * self.n), True
            g = self.opt(d, "g")
        else:
            A = ctx.assemble_rotation(1.0 / gc.OM)
            eps, drift, c, c_shared, g = o["eps"], (1.0, 1.0), self.up(d["c"]), bool(o.get("c_shared")), None
        if self.case.sweep == "forward":
            u, src = self.traj0(d["u0"]), self.opt(d, "src")
            if g is not None:
                return (lambda: ctx.linear_forward_react(A, src, g, u, NT, dt, eps, batch=B)), [u]
            if self.case.entry_call == "raw":
                return (lambda: lib.check(ctx.handle, lib.lib.femfct_solidbody_forward(
                    ctx.handle, dptr(A), dptr(c), int(c_shared), dptr(u), NT, dt, eps, 1.0, drift[0], drift[1], B))), [u]
            return (lambda: ctx.solidbody_forward(A, c, u, NT, dt, eps, 1.0, drift, B, c_shared, src_traj=src)), [u]
        u, uhat, p, mode = self.up(d["u"]), self.up(d["uhat"]), self.zeros(), o["mode"]
        if mode in ("finaltime", "alltime"):
            if g is not None:
                return (lambda: ctx.linear_adjoint_react(A, g, u, uhat, p, NT, dt, eps, alltime=mode == "alltime", batch=B)), [p]
            return (lambda: ctx.solidbody_adjoint(A, c, u, uhat, p, NT, dt, eps, 1.0, drift, mode == "alltime", B, c_shared)), [p]
        theta, tau, window = self.up(d["theta_u"]), d["tau_u"], self.opt(d, "window")
        if mode == "snapshots":
            if g is not None:
                return (lambda: ctx.linear_adjoint_react_obs(A, g, u, uhat, theta, tau, window, p, NT, dt, eps, batch=B)), [p]
            return (lambda: ctx.solidbody_adjoint_obs(A, c, u, uhat, theta, tau, window, p, NT, dt, eps, 1.0, drift, B,
                                                      c_shared)), [p]
        lo, hi, sigma, ws = self.up(d["lower"]), self.up(d["upper"]), self.up(d["sigma"]), self.opt(d, "window_s")
        if g is not None:
            return (lambda: ctx.linear_adjoint_react_bounds(A, g, u, uhat, theta, tau, window, lo, hi, gc.GAMMA, sigma, ws, p,
                                                            NT, dt, eps, batch=B)), [p]
        return (lambda: ctx.solidbody_adjoint_bounds(A, c, u, uhat, theta, tau, window, lo, hi, gc.GAMMA, sigma, ws, p, NT, dt,
                                                     eps, 1.0, drift, B, c_shared)), [p]

    def _linear(self, d):
        return self._solidbody(d, linear=True)

    def _obs(self, d, two):
        if self.case.opts["mode"] != "snapshots":
            return None
        return self.dev.DeviceObs(theta_u=self.up(d["theta_u"]), tau_u=d["tau_u"],
                                  theta_v=self.up(d["theta_v"]) if two else None, tau_v=d["tau_v"] if two else 0.0,
                                  window=self.opt(d, "window"))

    def _nonlinear(self, d):
        ctx, o, B, dt = self.ctx, self.case.opts, self.B, d["dt"]
        eps, _, wind = self.systems.get_nonlinear_eqns_params()
        Aw, _ = self.S.convection(wind, "nonlinear")
        if self.case.sweep == "forward":
            u = self.traj0(d["u0"])
            if o.get("ct"):
                c = self.up(d["c"])
                return (lambda: ctx.nonlinear_forward_ct(Aw, c, u, NT, dt, eps, batch=B)), [u]
            c1 = self.up(d["c"][:, 1])
            return (lambda: ctx.nonlinear_forward(Aw, c1, u, NT, dt, eps, batch=B)), [u]
        u, uhat, p, obs = self.up(d["u"]), self.up(d["uhat"]), self.zeros(), self._obs(d, False)
        return (lambda: ctx.nonlinear_adjoint(Aw, u, uhat, p, NT, dt, eps, batch=B, alltime=o["mode"] == "alltime", obs=obs)), [p]

    def _schnak(self, d):
        ctx, o, B, dt, lib, dptr = self.ctx, self.case.opts, self.B, d["dt"], self.hp._lib, self.dev.dptr
        par, wind = self.systems._schnak_par()
        par = np.asarray(par, dtype=np.float64)
        Aw, AwT = self.S.convection(wind, "schnak")
        ws = d.get("wind_scale")
        if self.case.sweep == "forward":
            u, v = self.traj0(d["u0"]), self.traj0(d["v0"])
            if o.get("ct"):
                c = self.up(d["c"])
                return (lambda: ctx.schnak_forward_ct(Aw, c, u, v, NT, dt, par, 1.0, batch=B, wind_scale=ws)), [u, v]
            c1 = self.up(d["c"][:, 1])
            if self.case.entry_call == "raw":
                return (lambda: lib.check(ctx.handle, lib.lib.femfct_schnak_forward(
                    ctx.handle, dptr(Aw), dptr(c1), dptr(u), dptr(v), NT, dt, _host(par), 1.0, B))), [u, v]
            return (lambda: ctx.schnak_forward(Aw, c1, u, v, NT, dt, par, 1.0, batch=B, wind_scale=ws)), [u, v]
        u, v, uhat, vhat = self.up(d["u"]), self.up(d["v"]), self.up(d["uhat"]), self.up(d["vhat"])
        p, q, alltime, obs = self.zeros(), self.zeros(), o["mode"] == "alltime", self._obs(d, True)
        if self.case.entry_call == "raw":
            return (lambda: lib.check(ctx.handle, lib.lib.femfct_schnak_adjoint(
                ctx.handle, dptr(AwT), dptr(u), dptr(v), dptr(uhat), dptr(vhat), dptr(p), dptr(q), NT, dt, _host(par),
                int(alltime), B))), [p, q]
        return (lambda: ctx.schnak_adjoint(AwT, u, v, uhat, vhat, p, q, NT, dt, par, batch=B, alltime=alltime, wind_scale=ws,
                                           obs=obs)), [p, q]

    def _chtxs(self, d):
        ctx, o, B, dt = self.ctx, self.case.opts, self.B, d["dt"]
        cpar = self.systems._chtxs_par()
        growth = gc.GROWTH if o.get("growth") else None
        if self.case.sweep == "forward":
            u, v = self.traj0(d["u0"]), self.traj0(d["v0"])
            if o.get("ct"):
                c = self.up(d["c"])
                return (lambda: ctx.chtxs_forward_ct(c, u, v, NT, dt, cpar, 0.1, batch=B, growth=growth)), [u, v]
            c1 = self.up(d["c"][:, 1])
            return (lambda: ctx.chtxs_forward(c1, u, v, NT, dt, cpar, 0.1, batch=B, growth=growth)), [u, v]
        u, v, uhat, vhat, c = self.up(d["u"]), self.up(d["v"]), self.up(d["uhat"]), self.up(d["vhat"]), self.up(d["c"])
        p, q, obs = self.zeros(), self.zeros(), self._obs(d, True)
        return (lambda: ctx.chtxs_adjoint(u, v, uhat, vhat, p, q, c, NT, dt, cpar, 0.1, alltime=o["mode"] == "alltime", batch=B,
                                          growth=growth, obs=obs, misfit=o.get("misfit", "mass"))), [p, q]

    def run(self, d):
        call, outs = self.sweep(d)
        for _ in range(2):                              # the second sweep runs at the settled budget
            call()
        res = {name: a.download().reshape(self.B, NT + 1, self.n) for name, a in zip(d["outputs"], outs)}
        logs = {"step." + k: v for k, v in self.ctx.traj_info(NT, self.B).items()}
        if self.case.family in gc.SPECIES:
            logs.update({"species." + k: v for k, v in self.ctx.traj_krylov_info(NT, self.B).items()})
        return res, logs


def _variant(hp, systems, monkeypatch, case, rid, name, d):
    N, order, B, regime, _, species = REGIMES[rid]
    graphs, per_graph, profiling = VARIANTS[name]
    if per_graph is None:
        monkeypatch.delenv("FEMFCT_STEPS_PER_GRAPH", raising=False)
    else:
        monkeypatch.setenv("FEMFCT_STEPS_PER_GRAPH", per_graph)     # read in femfct_create
    R = _Run(hp, systems, case, N, order, B, species)
    try:
        if regime_knobs_default():
            assert R.ctx.kernel_regime(B) in [getattr(hp._lib, "REGIME_" + r) for r in regime], R.ctx.kernel_regime(B)
        R.ctx.set_graphs(graphs)
        if profiling:
            R.ctx.set_profiling(True)
        assert R.ctx.graph_replay_active() == (graphs and not profiling)
        return R.run(d)
    finally:
        R.close()


def _check_written_levels(case, d, res, name):
    for var, a in res.items():
        assert np.isfinite(a).all(), (name, var)
        peak = np.abs(a).max(axis=2)                    # (B, NT + 1)
        if case.sweep == "forward":
            assert np.all(peak[:, 1:] > 0), (name, var, peak)
        else:
            assert np.all(peak[:, :NT] > 0), (name, var, peak)
            assert np.all((peak[:, NT] > 0) == d["terminal"][var]), (name, var, peak[:, NT])


@pytest.mark.parametrize("rid, case_id", PARAMS)
def test_sweep_bits_do_not_depend_on_the_graph_chunking(hp, systems, monkeypatch, rid, case_id):
    """The sweep ``case_id`` in the regime ``rid`` under every variant of VARIANTS against eager stepping: the same bits in
    every output trajectory and every field of the step log (and of the species log), outputs finite and non-zero at
    every level the sweep writes."""
    case = gc.BY_ID[case_id]
    N, _, B = REGIMES[rid][:3]
    d = gc.inputs(case, N, B)
    names = list(VARIANTS)
    ref, ref_logs = _variant(hp, systems, monkeypatch, case, rid, names[0], d)
    _check_written_levels(case, d, ref, names[0])
    assert not np.any(ref_logs["step.flags"] & hp.FLAG_SOLVER_BUDGET)
    bad = []
    for name in names[1:]:
        res, logs = _variant(hp, systems, monkeypatch, case, rid, name, d)
        _check_written_levels(case, d, res, name)
        for var in ref:
            if not np.array_equal(res[var], ref[var]):
                lv = sorted({int(l) for l in np.argwhere(res[var] != ref[var])[:, 1]})
                bad.append(f"{name}: {var} differs at levels {lv}, rel l2 {rel(res[var], ref[var]):.3e}")
        assert sorted(logs) == sorted(ref_logs)
        for k in ref_logs:
            if not np.array_equal(logs[k], ref_logs[k]):
                steps = sorted({int(s) for s in np.argwhere(logs[k] != ref_logs[k])[:, 0]})
                bad.append(f"{name}: log {k} differs at steps {steps}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------- anchors at the default knob value
ANCHOR_NT, ANCHOR_N = 53, 21
ANCHOR_KNOBS = (None, "64")         # the default (graphs of 50 + 3 steps) and one graph


def _set_knob(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("FEMFCT_STEPS_PER_GRAPH", raising=False)
    else:
        monkeypatch.setenv("FEMFCT_STEPS_PER_GRAPH", value)


def _oracle_mesh(a1, a2):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    mesh = SquareMesh(a1, a2, ANCHOR_N - 1)
    return mesh, P1Assembler(mesh)


def _to_dev(a, n, v2d):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a.reshape(-1, n)[:, v2d]).reshape(a.shape)


def _from_dev(a, n, v2d):
    o = np.empty((a.size // n, n))
    o[:, v2d] = a.reshape(-1, n)
    return o.reshape(a.shape)


def test_anchor_solidbody_snapshots_and_bounds_53_steps_vs_oracle(hp, monkeypatch):
    """53 steps at the default FEMFCT_STEPS_PER_GRAPH (a graph of 50 steps and one of 3), N = 21, vertex order, graphs on:
    the forward sweep and the adjoint with snapshots at the levels 2, 49, 50, 51 and 53 and state bounds penalised at 10,
    49, 50 and 53 (not at 51), against oracle.traj.solidbody_forward and state_bounds_oracle.adjoint: STATE_TOL, ADJ_TOL.
    The same as one graph (FEMFCT_STEPS_PER_GRAPH=64) meets the same bars; both errors are printed side by side."""
    from oracle import traj as otraj
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    Nt, dt = ANCHOR_NT, 1e-3 * 80 / (ANCHOR_N - 1)
    mesh, asm = _oracle_mesh(-1.0, 1.0)
    n, v2d = mesh.nodes, mesh.vertex_to_dof
    tl = (Nt + 1) * n
    rng = np.random.default_rng(53)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    sb = otraj.SolidBody(asm, om=gc.OM)
    ck = 2.0 * rng.random(tl)
    uk = np.zeros(tl)
    uk[:n] = np.exp(-10 * ((x + 0.3) ** 2 + (y - 0.2) ** 2)) + 0.05 * rng.random(n)
    otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
    obs = solvers.Observations(Nt, [2, 49, 50, 51, Nt], [0.7, 1.1, 0.6, 0.9, 1.3])
    bounds = solvers.StateBounds(Nt, lower=0.02, upper=0.5, gamma=20.0, levels=[10, 49, 50, Nt], weights=[0.8, 1.2, 0.5, 0.9])
    sigma = bounds.sigma(dt)
    assert np.all(sigma[[49, 50, Nt]] != 0) and sigma[51] == 0 and obs.theta[51] != 0
    uhat = np.full(tl, np.nan)
    for lv in obs.levels:
        uhat[lv * n:(lv + 1) * n] = 0.8 * uk[lv * n:(lv + 1) * n] + 0.02 * np.cos(2 * x) * np.sin(y + lv)
    for lv in np.flatnonzero(sigma):                    # every penalised level has violated nodes on both sides
        u_lv = uk[lv * n:(lv + 1) * n]
        assert (u_lv < 0.02).any() and (u_lv > 0.5).any()
    pk_o = sbo.adjoint(sb, ck, uk, uhat, obs, bounds, n, Nt, dt)
    errs = {}
    for knob in ANCHOR_KNOBS:
        _set_knob(monkeypatch, knob)
        prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, ANCHOR_N - 1), Nt, dt, om=gc.OM, order=hp.ORDER_VERTEX)
        try:
            if regime_knobs_default():
                assert prob.ctx.kernel_regime(1) == hp._lib.REGIME_MESH
            assert prob.ctx.graph_replay_active()
            u_d = np.zeros(tl)
            u_d[:n] = _to_dev(uk[:n], n, v2d)
            prob.solve_state(_to_dev(ck, n, v2d), u_d)
            assert not np.any(prob.solver_log(1)["flags"] & hp.FLAG_SOLVER_BUDGET)
            p_d = prob.solve_adjoint(_to_dev(ck, n, v2d), _to_dev(uk, n, v2d), _to_dev(uhat, n, v2d), np.zeros(tl),
                                     optim="snapshots", obs=obs, state_bounds=bounds)
            assert not np.any(prob.solver_log(1)["flags"] & hp.FLAG_SOLVER_BUDGET)
        finally:
            prob.close()
        errs[knob] = (rel(_from_dev(u_d, n, v2d), uk), rel(_from_dev(p_d, n, v2d), pk_o))
    (eu, ep), (eu1, ep1) = errs[None], errs["64"]
    print(f"[graph chunks] solid body N={ANCHOR_N} {Nt} steps, rel l2 vs the oracle: forward 50+3 {eu:.3e} | one graph "
          f"{eu1:.3e}; snapshot + bounds adjoint 50+3 {ep:.3e} | one graph {ep1:.3e}")
    assert eu < STATE_TOL and eu1 < STATE_TOL, errs
    assert ep < ADJ_TOL and ep1 < ADJ_TOL, errs


def test_anchor_chemotaxis_growth_per_step_control_53_steps_vs_oracle(hp, systems, monkeypatch):
    """53 steps at the default FEMFCT_STEPS_PER_GRAPH (50 + 3), N = 21, vertex order, graphs on: the chemotaxis forward
    sweep with the per-step control and growth against chtxs_growth_oracle.solve_chtxs_system, and the snapshot adjoint
    with growth (u and v observed at the levels 2, 50 and 53) against systems_snapshots_oracle: STATE_TOL, ADJ_TOL.  The
    same as one graph (FEMFCT_STEPS_PER_GRAPH=64) meets the same bars; both errors are printed side by side."""
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    DeviceObs = importlib.import_module("fem-fct-pdeco_amd.device").DeviceObs
    Nt, dt, growth = ANCHOR_NT, 5e-4, gc.GROWTH
    mesh, asm = _oracle_mesh(0.0, 1.0)
    n, v2d = mesh.nodes, mesh.vertex_to_dof
    tl = (Nt + 1) * n
    rng = np.random.default_rng(5353)
    c = 20.0 * rng.random(tl)
    uo, vo = np.zeros(tl), np.zeros(tl)
    uo[:n] = 1.5 + 0.1 * (0.5 - rng.random(n))
    vo[:n] = 1.5 + 0.1 * (0.5 - rng.random(n))
    go.solve_chtxs_system(c, uo, vo, asm, n, Nt, dt, rescaling=0.1, growth=growth, per_step=True)
    obs_u = solvers.Observations(Nt, [2, 50, Nt], [1.0, 0.5, 0.8])
    obs_v = solvers.Observations(Nt, [2, 50, Nt], [0.6, 1.2, 0.7])
    uhat, vhat = np.full(tl, np.nan), np.full(tl, np.nan)
    for lv in (2, 50, Nt):
        uhat[lv * n:(lv + 1) * n] = 0.9 * uo[lv * n:(lv + 1) * n] + 0.02 * rng.random(n)
        vhat[lv * n:(lv + 1) * n] = 1.05 * vo[lv * n:(lv + 1) * n] + 0.02 * rng.random(n)
    po, qo = sso.solve_adjoint_chtxs_system(uo, vo, uhat, vhat, np.zeros(tl), np.zeros(tl), c, Nt * dt, asm, n, Nt, dt,
                                            (obs_u, obs_v), misfit="mass", rescaling=0.1, growth=growth)
    cpar = systems._chtxs_par()
    errs = {}
    for knob in ANCHOR_KNOBS:
        _set_knob(monkeypatch, knob)
        S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, ANCHOR_N - 1), order=hp.ORDER_VERTEX)
        ctx = S.ctx
        try:
            if regime_knobs_default():
                assert ctx.kernel_regime(1) == hp._lib.REGIME_MESH
            assert ctx.graph_replay_active()
            up = lambda a: ctx.array(_to_dev(a, n, v2d))
            z0 = lambda a: np.concatenate([a[:n], np.zeros(tl - n)])
            d_c, d_u, d_v = up(c), up(z0(uo)), up(z0(vo))
            ctx.chtxs_forward_ct(d_c, d_u, d_v, Nt, dt, cpar, 0.1, batch=1, growth=growth)
            for log in (ctx.traj_info(Nt, 1), ctx.traj_krylov_info(Nt, 1)):
                assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET)
            u_d, v_d = d_u.download(), d_v.download()
            dobs = DeviceObs(theta_u=ctx.array(obs_u.theta), tau_u=obs_u.tau, theta_v=ctx.array(obs_v.theta), tau_v=obs_v.tau)
            d_p, d_q = ctx.zeros(tl), ctx.zeros(tl)
            ctx.chtxs_adjoint(up(uo), up(vo), up(uhat), up(vhat), d_p, d_q, d_c, Nt, dt, cpar, 0.1, batch=1, growth=growth,
                              obs=dobs, misfit="mass")
            for log in (ctx.traj_info(Nt, 1), ctx.traj_krylov_info(Nt, 1)):
                assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET)
            p_d, q_d = d_p.download(), d_q.download()
        finally:
            S.close()
        errs[knob] = tuple(rel(_from_dev(a, n, v2d), b) for a, b in ((u_d, uo), (v_d, vo), (p_d, po), (q_d, qo)))
    fmt = lambda e: "u {:.3e} v {:.3e} p {:.3e} q {:.3e}".format(*e)
    print(f"[graph chunks] chemotaxis growth N={ANCHOR_N} {Nt} steps, rel l2 vs the oracle: 50+3 {fmt(errs[None])} | one graph "
          f"{fmt(errs['64'])}")
    for e in errs.values():
        assert max(e[:2]) < STATE_TOL and max(e[2:]) < ADJ_TOL, errs
