"""All-time adjoint of the nonlinear equation on the GPU (-m gpu): femfct_nonlinear_adjoint_alltime,
``solve_adjoint_nonlinear_equation(optim="alltime")`` and ``SystemPDECO("nonlinear", optim="alltime")``, against the CPU
reference of tests/nonlinear_alltime_oracle.py (states from the per-step CPU chain of tests/per_step_oracle.py).
UnitSquare 41 x 41, dt = 5e-4, 50 steps, unless a test says otherwise; the last test runs the size of
nonlinear_FCT_PDECO_alltime.py (dt = 1e-3, T = 0.5: 500 + 500 steps)."""
import importlib

import numpy as np
import pytest

import nonlinear_alltime_oracle as na
import per_step_oracle as po

pytestmark = pytest.mark.gpu

NC, NT, DT = 40, 50, 5e-4


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def asm():
    from oracle.assembly import P1Assembler
    from oracle.mesh import SquareMesh
    return P1Assembler(SquareMesh(0.0, 1.0, NC))


@pytest.fixture(scope="module")
def V(hp):
    return hp.SquareMeshP1(0.0, 1.0, NC)


@pytest.fixture
def system(hp, V):
    systems = importlib.import_module("fem-fct-pdeco_amd.systems")
    made = []

    def make(mesh=None):
        S = systems.PDESystems(mesh or V, order=hp._lib.ORDER_VERTEX)
        made.append(S)
        return S
    yield make
    for S in made:
        S.close()


def relmax(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def _report(name, **vals):
    print(f"[all-time] {name}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}"
                                             for k, v in vals.items()))


def cpu_forward(asm, c, num_steps=NT, dt=DT, scale=1.0):
    n = asm.mesh.nodes
    u = np.zeros((num_steps + 1) * n)
    u[:n] = scale * po.initial_conditions("nonlinear", asm.mesh)[0]
    po.solve_nonlinear_equation(c, u, None, asm, n, num_steps, dt)
    return u


def cpu_adjoint(asm, u, uhat, num_steps=NT, dt=DT):
    n = asm.mesh.nodes
    return na.solve_adjoint_nonlinear_equation(u, uhat, np.zeros_like(u), num_steps * dt, asm, n, num_steps, dt)


class Dev:
    """C ABI calls of one PDESystems in the device's vertex order; host arrays in FEniCS DoF order, one row per member"""

    def __init__(self, S, num_steps=NT, dt=DT):
        self.S, self.ctx, self.n, self.Nt, self.dt = S, S.ctx, S.n, num_steps, dt
        self.v2d = np.asarray(S.mesh.vertex_to_dof)
        systems = importlib.import_module("fem-fct-pdeco_amd.systems")
        self.eps, _, w = systems.get_nonlinear_eqns_params()
        self.Aw, _ = S.convection(w, "nonlinear")

    def up(self, rows):
        rows = np.atleast_2d(rows)
        return self.ctx.array(np.ascontiguousarray(rows.reshape(-1, self.n)[:, self.v2d]).ravel())

    def down(self, d, B):
        h = d.download().reshape(-1, self.n)
        out = np.empty_like(h)
        out[:, self.v2d] = h
        return out.reshape(B, -1)

    def forward(self, cs, u0s):
        """per-step forward sweep of B members: cs (B, tl) controls, u0s (B, n) initial states"""
        B, tl = len(u0s), (self.Nt + 1) * self.n
        init = np.zeros((B, tl))
        init[:, :self.n] = u0s
        c, u = self.up(cs), self.up(init)
        try:
            self.ctx.nonlinear_forward_ct(self.Aw, c, u, self.Nt, self.dt, self.eps, batch=B)
            return self.down(u, B)
        finally:
            c.free()
            u.free()

    def adjoint(self, us, uhats, alltime=True, shared=False):
        """B = len(us) members; uhats: (B, tl) trajectories, one row with shared, or (B, n) final-time targets"""
        B = len(us)
        u, tg = self.up(us), self.up(uhats)
        p = self.ctx.array(np.full(B * (self.Nt + 1) * self.n, np.nan))     # every level must be written
        try:
            self.ctx.nonlinear_adjoint(self.Aw, u, tg, p, self.Nt, self.dt, self.eps, batch=B, alltime=alltime,
                                       uhat_shared=shared)
            return self.down(p, B)
        finally:
            for d in (u, tg, p):
                d.free()


def _control(asm, amp=0.5, phase=0.0):
    return po.varying_control(po.bump(asm.mesh), NT, amp=amp, phase=phase)


@pytest.fixture(scope="module")
def case(asm):
    """a state at a varying per-step control and a target trajectory at another one (CPU chain), the CPU adjoint"""
    u = cpu_forward(asm, _control(asm))
    uhat = cpu_forward(asm, _control(asm, amp=0.5, phase=0.3) + 0.3 * na.sinsin_control(asm.mesh, NT))
    return u, uhat, cpu_adjoint(asm, u, uhat)


# ----------------------------------------------------------------------------- 1. device vs CPU reference
@pytest.mark.parametrize("path", ["default", "tile", "no_graphs"])
def test_alltime_adjoint_vs_cpu_reference(hp, system, monkeypatch, case, path):
    if path == "tile":
        monkeypatch.setenv("FEMFCT_MESH_STEP", "0")
    S = system()
    if path == "tile":
        assert S.ctx.kernel_regime(1) != hp._lib.REGIME_MESH
    if path == "no_graphs":
        S.ctx.set_graphs(False)
    u, uhat, p_ref = case
    p = Dev(S).adjoint([u], [uhat])[0]
    err = relmax(p, p_ref)
    _report(f"path {path} (regime {S.ctx.kernel_regime(1)}) vs CPU reference", p=err, pmax=float(np.max(np.abs(p_ref))))
    assert np.max(np.abs(p_ref)) > 0 and err < 1e-10, err


# ----------------------------------------------------------------------------- 2. zero misfit
def test_own_forward_as_target_gives_zero_adjoint(asm, system):
    D = Dev(system())
    u = D.forward([_control(asm)], [po.initial_conditions("nonlinear", asm.mesh)[0]])
    p = D.adjoint(u, u.copy())
    _report("target = own forward trajectory", max_abs_p=float(np.max(np.abs(p))))
    assert np.all(p == 0.0)


# ----------------------------------------------------------------------------- 3. batches
@pytest.mark.parametrize("shared", [False, True])
def test_batch_members_equal_single_runs(asm, system, case, shared):
    B = 4
    S = system()
    D = Dev(S)
    u0 = po.initial_conditions("nonlinear", asm.mesh)[0]
    cs = np.stack([_control(asm, amp=0.2 + 0.1 * b, phase=2 * np.pi * b / B) for b in range(B)])
    us = D.forward(cs, np.stack([(1.0 + 0.1 * b) * u0 for b in range(B)]))
    _, uhat, _ = case
    uhats = uhat[None, :] if shared else np.stack([(1.0 - 0.05 * b) * uhat for b in range(B)])
    pb = D.adjoint(us, uhats, shared=shared)
    for b in range(B):
        one = D.adjoint(us[b:b + 1], uhats[0 if shared else b][None, :])[0]
        _report(f"B={B} {'shared' if shared else 'per-member'} target, member {b} vs B=1 (regime "
                f"{S.ctx.kernel_regime(B)} / {S.ctx.kernel_regime(1)})", bitwise=np.array_equal(pb[b], one),
                err=relmax(pb[b], one))
        assert np.array_equal(pb[b], one), b
    assert not np.array_equal(pb[0], pb[1])


# ----------------------------------------------------------------------------- 4. isolation, launch count
def test_final_time_and_alltime_sweeps_do_not_interfere(hp, asm, system, case):
    u, uhat, _ = case
    n = asm.mesh.nodes
    uT = uhat[NT * n:]

    fresh_ft = Dev(system()).adjoint([u], [uT], alltime=False)[0]
    fresh_at = Dev(system()).adjoint([u], [uhat])[0]
    D = Dev(system())
    at_then = D.adjoint([u], [uhat])
    ft_after = D.adjoint([u], [uT], alltime=False)[0]
    at_after = D.adjoint([u], [uhat])[0]
    _report("final-time after all-time vs fresh context", bitwise=np.array_equal(ft_after, fresh_ft),
            err=relmax(ft_after, fresh_ft))
    assert np.array_equal(ft_after, fresh_ft)
    assert np.array_equal(at_after, fresh_at) and np.array_equal(at_then[0], fresh_at)
    # the two sweeps really differ: a replayed graph of the other kind would show here
    assert relmax(ft_after, at_after) > 1e-3
    assert np.array_equal(fresh_ft[NT * n:], uT - u[NT * n:]) and np.all(fresh_at[NT * n:] == 0.0)


def test_alltime_sweep_launches_what_the_final_time_sweep_launches(hp, asm, system, case):
    u, uhat, _ = case
    n = asm.mesh.nodes
    D = Dev(system())
    D.adjoint([u], [uhat[NT * n:]], alltime=False)
    D.adjoint([u], [uhat])                                            # warm: budgets settled, nothing re-run below
    counts = {}
    for name, tg, at in (("final-time", uhat[NT * n:], False), ("all-time", uhat, True)):
        D.ctx.set_profiling(True)
        D.adjoint([u], [tg], alltime=at)
        rep = D.ctx.profile_report()
        D.ctx.set_profiling(False)
        counts[name] = {k: v[1] for k, v in rep.items()}
        _report(f"{name} sweep launches per class (regime {D.ctx.kernel_regime(1)})", **counts[name])
    assert counts["final-time"] == counts["all-time"]
    assert counts["all-time"]["assemble"] == NT


# ----------------------------------------------------------------------------- 5. public wrapper
def test_public_wrapper_alltime(hp, asm, V, case):
    u, uhat, p_ref = case
    n = V.nodes
    pk = np.zeros_like(u)
    out = hp.solve_adjoint_nonlinear_equation(u, uhat, pk, NT * DT, V, n, NT, DT, None, optim="alltime")
    assert out is pk
    err = relmax(pk, p_ref)
    _report("solve_adjoint_nonlinear_equation(optim='alltime') vs CPU reference", p=err)
    assert err < 1e-10, err
    # the default stays the final-time sweep of helpers.py
    from oracle import traj as otraj
    p_ft = hp.solve_adjoint_nonlinear_equation(u, uhat[NT * n:], np.zeros_like(u), NT * DT, V, n, NT, DT, None)
    ref_ft = otraj.solve_adjoint_nonlinear_equation(u, uhat[NT * n:], np.zeros_like(u), NT * DT, asm, n, NT, DT)
    assert relmax(p_ft, ref_ft) < 1e-10
    untouched = pk.copy()
    for bad in (dict(optim="sometimes"), dict(optim="alltime", tg=uhat[NT * n:]), dict(optim="finaltime", tg=uhat)):
        with pytest.raises(ValueError):
            hp.solve_adjoint_nonlinear_equation(u, bad.get("tg", uhat), pk, NT * DT, V, n, NT, DT, None, optim=bad["optim"])
        assert np.array_equal(pk, untouched)


# ----------------------------------------------------------------------------- 6. PGD loop
def _oracle_pgd(monkeypatch, asm, ic, targets, num_steps, dt, opts):
    from oracle import pdeco as opdeco, traj as otraj
    monkeypatch.setattr(otraj, "solve_nonlinear_equation", po.solve_nonlinear_equation)
    monkeypatch.setattr(otraj, "solve_adjoint_nonlinear_equation", na.solve_adjoint_nonlinear_equation)
    try:
        return opdeco.projected_gradient_descent("nonlinear", asm, asm.mass(), ic, targets, num_steps, dt, **opts)
    finally:
        monkeypatch.undo()


def test_pgd_loop_alltime_vs_oracle(hp, asm, V, monkeypatch):
    ic = po.initial_conditions("nonlinear", asm.mesh)
    targets = (cpu_forward(asm, _control(asm, amp=0.5, phase=0.3)),)
    opts = dict(optim="alltime", max_iter_GD=2, tol=0.0)
    ref = _oracle_pgd(monkeypatch, asm, ic, targets, NT, DT, opts)
    mref = [m for ms in ref["armijo_margin"] for m in ms]
    for speculative in (True, False):
        with hp.SystemPDECO("nonlinear", V, NT, DT, control_per_step=True, **opts) as prob:
            got = prob.run(ic, targets, speculative=speculative)
        mgot = [m for ms in got["armijo_margin"] for m in ms]
        cerr = np.linalg.norm(got["c"] - ref["c"]) / np.linalg.norm(ref["c"])
        _report(f"PGD all-time, {'speculative' if speculative else 'sequential'}: armijo_its {got['armijo_its']} "
                f"(oracle {ref['armijo_its']}), margins {['%.3e' % m for m in mgot]} (oracle {['%.3e' % m for m in mref]})",
                c=cerr, cost=relmax(np.array(got["cost"]), np.array(ref["cost"])))
        assert got["it"] == ref["it"] and got["armijo_its"] == ref["armijo_its"], (got["armijo_its"], ref["armijo_its"])
        np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9)
        assert cerr < 1e-8, cerr
    assert ref["cost"][-1] < ref["cost"][0]


# ----------------------------------------------------------------------------- 7. the script's size
def test_script_size_forward_adjoint_and_pgd(hp, system, monkeypatch):
    """nonlinear_FCT_PDECO_alltime.py:40-55: dx = 0.025, dt = 1e-3, T = 0.5; target from c = sin(2 pi x) sin(2 pi y)"""
    from oracle.assembly import P1Assembler
    from oracle.mesh import SquareMesh
    Nt, dt = 500, 1e-3
    asm41 = P1Assembler(SquareMesh(0.0, 1.0, 40))
    mesh, n = asm41.mesh, asm41.mesh.nodes
    ic = po.initial_conditions("nonlinear", mesh)
    uhat = cpu_forward(asm41, na.sinsin_control(mesh, Nt), Nt, dt)
    c = 0.5 * po.varying_control(po.bump(mesh), Nt)
    u_ref = cpu_forward(asm41, c, Nt, dt)
    p_ref = cpu_adjoint(asm41, u_ref, uhat, Nt, dt)
    D = Dev(system(), Nt, dt)
    u = D.forward([c], [ic[0]])
    p = D.adjoint(u, [uhat])[0]
    errs = dict(u=relmax(u[0], u_ref), p=relmax(p, p_ref))
    _report("script size: device forward + all-time adjoint vs CPU reference", **errs)
    assert max(errs.values()) < 1e-8, errs

    opts = dict(optim="alltime", max_iter_GD=2, tol=0.0)
    ref = _oracle_pgd(monkeypatch, asm41, ic, (uhat,), Nt, dt, opts)
    V41 = hp.SquareMeshP1(0.0, 1.0, 40)
    with hp.SystemPDECO("nonlinear", V41, Nt, dt, control_per_step=True, **opts) as prob:
        got = prob.run(ic, (uhat,), speculative=True)
    _report(f"script size PGD: armijo_its {got['armijo_its']} (oracle {ref['armijo_its']}), cost {got['cost']} "
            f"(oracle {ref['cost']})", cost=relmax(np.array(got["cost"]), np.array(ref["cost"])))
    assert got["it"] == ref["it"] and got["armijo_its"] == ref["armijo_its"]
    assert got["cost"][-1] < got["cost"][0]
