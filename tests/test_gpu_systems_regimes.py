"""The three PDE systems' sweeps in every kernel regime of the vertex order (-m gpu), against the CPU oracle.

The drop-in wrappers run the nonlinear, Schnakenberg and chemotaxis sweeps in vertex order (systems._system), where the
mesh size and the batch pick the kernels of the FCT step (femfct_kernel_regime) and of the species (non-FCT) solve:

  N = 6, B = 1       one-workgroup FCT step; n = 36: fewer nodes than one wave of the 1024-thread one-workgroup species
                     solve (k_mesh_cheb_solve<2>: thread t owns the nodes t and t + 1024)
  N = 32, B = 3      one-workgroup FCT step; n = 1024: the species solve's second node slot wholly empty
  N = 33, B = 1      one-workgroup FCT step at an odd N with a non-flux matrix; n = 1089: 65 threads own a second node
  N = 43, B = 1      smallest mesh on the 32-patch FCT step, species solve still one workgroup
  N = 45, B = 1 / 8  n = 2025: the largest one-workgroup species solve, 23 threads without a second node
  N = 46, B = 1      smallest mesh past the one-workgroup species solve (n <= 2048): tile Chebyshev, 32-patch FCT step
  N = 47, B = 8      single-patch species solve (N <= 48 and B >= 8: femfct_single_patch), 32-patch FCT step
  N = 61, B = 1 / 5  32-patch tiles; 61 is no multiple of any tile width.  femfct_tile_plan takes the fewest launches for
                     a sweep budget, and halos 11..13 only while t^2 * B <= wg_slots (256): at B = 1 every halo up to 13
                     qualifies (t = 11 tiles per side at H = 13), at B = 5 only up to 11 (H = 12: 64 * 5 > 256) -- a
                     budget of 24 sweeps runs as 2 launches of H = 12 at B = 1 and as 3 launches of H = 8 at B = 5
  N = 81, B = 13/14  both sides of the switch to the 64-patch kernels at n * B = 90 000
  N = 129, B = 1 / 6 the Mimura grid, 32-patch tiles alone, 64-patch kernels in a batch of six (Armijo trials)
  N = 301, B = 1     64-patch kernels on one mesh; 301 = 6 * 48 + 13 leaves a partial edge patch
  N = 301, walkers   the same with FEMFCT_T4_WALKERS=5: persistent walking Jacobi launches with the systems' operators

N is the number of nodes per side of the unit square.  Every case asserts the regime it claims (unless a tuning knob
moves it, see _regime_knobs_default), runs every sweep of one system on B members with their own data, compares the
members with the oracle (all of them for B <= 8, else the first, middle and last one) and with the same member run
alone (another regime for B > 1: the solver tolerance, not bits), and checks the solver logs."""
import importlib

import numpy as np
import pytest

import nonlinear_alltime_oracle as na
import per_step_oracle as pso
from regime_helpers import REGIME_KNOBS, regime_knobs_default as _regime_knobs_default  # noqa: F401

pytestmark = pytest.mark.gpu

STATE_TOL, ADJ_TOL, MEMBER_TOL = 1e-10, 1e-9, 1e-12
DT = {"nonlinear": 1e-3, "schnak": 5e-4, "chtxs": 5e-4}


CASES = [
    pytest.param(6, 1, "MESH", {}, id="N6-B1"),
    pytest.param(32, 3, "MESH", {}, id="N32-B3-second-slot-empty"),
    pytest.param(33, 1, "MESH", {}, id="N33-B1-second-slot-65"),
    pytest.param(43, 1, "TILE32", {}, id="N43-B1"),
    pytest.param(45, 1, "TILE32", {}, id="N45-B1-largest-one-workgroup-species"),
    pytest.param(45, 8, "TILE32", {}, id="N45-B8-largest-one-workgroup-species"),
    pytest.param(46, 1, "TILE32", {}, id="N46-B1"),
    pytest.param(47, 8, "TILE32", {}, id="N47-B8-single-patch"),
    pytest.param(61, 1, "TILE32", {}, id="N61-B1-deep-halo"),
    pytest.param(61, 5, "TILE32", {}, id="N61-B5"),
    pytest.param(81, 13, "TILE32", {}, id="N81-B13"),
    pytest.param(81, 14, "PATCH64", {}, id="N81-B14"),
    pytest.param(129, 1, "TILE32", {}, id="N129-B1"),
    pytest.param(129, 6, "PATCH64", {}, id="N129-B6"),
    pytest.param(301, 1, "PATCH64", {}, id="N301-B1"),
    pytest.param(301, 1, "PATCH64", {"FEMFCT_T4_WALKERS": "5"}, id="N301-B1-walkers5"),
]


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


def _report(name, **errs):
    print(f"[regimes] {name}: " + ", ".join(f"{k}={v:.3e}" for k, v in errs.items()))


def _num_steps(N):
    return 2 if N >= 301 else (3 if N >= 129 else 4)


_ASM = {}


def _oracle(N):
    """(mesh, assembler) of the oracle on the unit square with N nodes per side, kept for the module"""
    if N not in _ASM:
        from oracle.mesh import SquareMesh
        from oracle.assembly import P1Assembler
        mesh = SquareMesh(0.0, 1.0, N - 1)
        _ASM.clear()                       # one mesh at a time (the cases come grouped by N)
        _ASM[N] = (mesh, P1Assembler(mesh))
    return _ASM[N]


# the oracle's results per (system, N, member, sweep): the cases that share a mesh share members
_ORACLE = {}


def _cached(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


class _Members:
    """Per-member host data in vertex order (the device's), and the conversions to the oracle's FEniCS DoF order."""

    def __init__(self, system, N, B, Nt):
        mesh, _ = _oracle(N)
        self.n, self.Nt, self.B = mesh.nodes, Nt, B
        self.tl = (Nt + 1) * self.n
        self.v2d = mesh.vertex_to_dof
        x, y = mesh.x, mesh.y                                    # vertex order
        self.x, self.y = x, y
        self.rngs = [np.random.default_rng([N, m, {"nonlinear": 0, "schnak": 1, "chtxs": 2}[system]]) for m in range(B)]

    def to_dof(self, a):
        a = np.asarray(a)
        out = np.empty_like(a.reshape(-1, self.n))
        out[:, self.v2d] = a.reshape(-1, self.n)
        return out.reshape(a.shape)

    def traj(self, x0s):
        """B trajectories with their first level set (B x tl)"""
        a = np.zeros((len(x0s), self.tl))
        a[:, :self.n] = np.asarray(x0s)
        return a


def _check_logs(hp, log, cheb):
    assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET), log["flags"]
    assert log["solver_resid"].max() <= 1e-13, log["solver_resid"].max()
    if cheb:
        assert np.all(log["flags"] & hp.FLAG_CHEBYSHEV), log["flags"]


class _Device:
    """Runs a sweep on B members (or one member alone) and checks both solver logs after it."""

    def __init__(self, hp, ctx, Nt, species, cheb):
        self.hp, self.ctx, self.Nt, self.species, self.cheb = hp, ctx, Nt, species, cheb

    def run(self, sweep, outs, ins, B):
        """sweep(device inputs..., device outputs..., batch) with host arrays (B x ...); returns the outputs (B x tl)"""
        d_in = [self.ctx.array(np.ascontiguousarray(a).ravel()) for a in ins]
        d_out = [self.ctx.array(np.ascontiguousarray(a).ravel()) for a in outs]
        try:
            sweep(*d_in, *d_out, B)
            _check_logs(self.hp, self.ctx.traj_info(self.Nt, B), False)
            if self.species:
                _check_logs(self.hp, self.ctx.traj_krylov_info(self.Nt, B), self.cheb)
            return [d.download().reshape(B, -1) for d in d_out]
        finally:
            for d in d_in + d_out:
                d.free()


def _compare(name, D, mem, sweep, outs, ins, oracle, tol, errs):
    """Batched run of ``sweep``, every member alone at B = 1, and the oracle on the members it checks.
    oracle(m) -> the member's outputs in DoF order.  Records the worst errors under ``name``."""
    B = mem.B
    got = D.run(sweep, outs, ins, B)
    e_or, e_one = 0.0, 0.0
    for m in (range(B) if B <= 8 else sorted({0, B // 2, B - 1})):
        for g, o in zip(got, oracle(m)):
            e_or = max(e_or, rel(mem.to_dof(g[m]), o))
    if B > 1:
        for m in range(B):
            one = D.run(sweep, [a[m:m + 1] for a in outs], [a[m:m + 1] for a in ins], 1)
            for g, o in zip(got, one):
                e_one = max(e_one, rel(g[m], o[0]))
        assert e_one < MEMBER_TOL, (name, e_one)
    errs[name] = e_or
    if B > 1:
        errs[name + "_vs_alone"] = e_one
    assert e_or < tol, (name, e_or)
    return got


def _nonlinear(hp, systems, S, D, mem, N, dt):
    from oracle import traj as otraj
    _, asm = _oracle(N)
    ctx, n, Nt, tl, B = S.ctx, mem.n, mem.Nt, mem.tl, mem.B
    eps, _, wind = systems.get_nonlinear_eqns_params()
    Aw, _ = S.convection(wind, "nonlinear")
    x, y = mem.x, mem.y
    u0 = [5 * y * (y - 1) * x * (x - 1) * np.sin(4 * np.pi * x) + 0.05 * r.random(n) for r in mem.rngs]
    c = np.stack([r.random(tl) for r in mem.rngs])                    # its own control trajectory per member
    errs = {}

    def o_fwd(m, per_step):
        def f():
            uo = np.zeros(tl)
            uo[:n] = mem.to_dof(u0[m])
            (pso if per_step else otraj).solve_nonlinear_equation(mem.to_dof(c[m]), uo, None, asm, n, Nt, dt)
            return [uo]
        return _cached(("nonlinear", N, m, "fwd_ct" if per_step else "fwd"), f)

    c1 = c[:, n:2 * n]
    (u,) = _compare("u", D, mem, lambda c_, u_, b: ctx.nonlinear_forward(Aw, c_, u_, Nt, dt, eps, batch=b),
                    [mem.traj(u0)], [c1], lambda m: o_fwd(m, False), STATE_TOL, errs)
    _compare("u_ct", D, mem, lambda c_, u_, b: ctx.nonlinear_forward_ct(Aw, c_, u_, Nt, dt, eps, batch=b),
             [mem.traj(u0)], [c], lambda m: o_fwd(m, True), STATE_TOL, errs)
    uhat_T = np.stack([0.8 * u[m, Nt * n:] + 0.05 * r.random(n) for m, r in enumerate(mem.rngs)])
    uhat = np.stack([0.8 * u[m] + 0.05 * r.random(tl) for m, r in enumerate(mem.rngs)])

    def o_adj(m, alltime):
        def f():
            po = np.zeros(tl)
            if alltime:
                na.solve_adjoint_nonlinear_equation(mem.to_dof(u[m]), mem.to_dof(uhat[m]), po, Nt * dt, asm, n, Nt, dt)
            else:
                otraj.solve_adjoint_nonlinear_equation(mem.to_dof(u[m]), mem.to_dof(uhat_T[m]), po, Nt * dt, asm, n, Nt, dt)
            return [po]
        return f()

    _compare("p_final", D, mem, lambda u_, t_, p_, b: ctx.nonlinear_adjoint(Aw, u_, t_, p_, Nt, dt, eps, batch=b),
             [np.zeros((B, tl))], [u, uhat_T], lambda m: o_adj(m, False), ADJ_TOL, errs)
    p = _compare("p_all", D, mem,
                 lambda u_, t_, p_, b: ctx.nonlinear_adjoint(Aw, u_, t_, p_, Nt, dt, eps, batch=b, alltime=True),
                 [np.zeros((B, tl))], [u, uhat], lambda m: o_adj(m, True), ADJ_TOL, errs)[0]
    assert np.abs(p[:, :Nt * n]).max() > 0
    return errs


def _schnak(hp, systems, S, D, mem, N, dt):
    from oracle import traj as otraj
    _, asm = _oracle(N)
    ctx, n, Nt, tl, B = S.ctx, mem.n, mem.Nt, mem.tl, mem.B
    par, wind = systems._schnak_par()
    Aw, AwT = S.convection(wind, "schnak")
    x, y = mem.x, mem.y
    u0 = [1.0 + 0.1 * np.cos(2 * np.pi * (x + y)) + 0.02 * r.random(n) for r in mem.rngs]
    v0 = [0.9 + 0.1 * np.cos(2 * np.pi * (x - y)) + 0.02 * r.random(n) for r in mem.rngs]
    c = np.stack([0.1 + 0.05 * r.random(tl) for r in mem.rngs])

    def s(t):                                                         # separable wind s(t) w0(x)
        return 1.5 * np.cos(40.0 * t) - 0.25
    ws = systems._wind_factors(s, Nt, dt)
    errs = {}

    def o_fwd(m, mode):
        def f():
            uo, vo = np.zeros(tl), np.zeros(tl)
            uo[:n], vo[:n] = mem.to_dof(u0[m]), mem.to_dof(v0[m])
            if mode == "ct":
                pso.solve_schnak_system(mem.to_dof(c[m]), uo, vo, asm, n, Nt, dt)
            else:
                otraj.solve_schnak_system(mem.to_dof(c[m]), uo, vo, asm, n, Nt, dt, wind_scale=s if mode == "wind" else None)
            return [uo, vo]
        return _cached(("schnak", N, m, mode), f)

    c1 = c[:, n:2 * n]
    u, v = _compare("uv", D, mem, lambda c_, u_, v_, b: ctx.schnak_forward(Aw, c_, u_, v_, Nt, dt, par, 1.0, batch=b),
                    [mem.traj(u0), mem.traj(v0)], [c1], lambda m: o_fwd(m, "frozen"), STATE_TOL, errs)
    _compare("uv_wind", D, mem,
             lambda c_, u_, v_, b: ctx.schnak_forward(Aw, c_, u_, v_, Nt, dt, par, 1.0, batch=b, wind_scale=ws),
             [mem.traj(u0), mem.traj(v0)], [c1], lambda m: o_fwd(m, "wind"), STATE_TOL, errs)
    _compare("uv_ct", D, mem, lambda c_, u_, v_, b: ctx.schnak_forward_ct(Aw, c_, u_, v_, Nt, dt, par, 1.0, batch=b),
             [mem.traj(u0), mem.traj(v0)], [c], lambda m: o_fwd(m, "ct"), STATE_TOL, errs)
    rs = mem.rngs
    uhat_T = np.stack([0.9 * u[m, Nt * n:] + 0.02 * rs[m].random(n) for m in range(B)])
    vhat_T = np.stack([1.1 * v[m, Nt * n:] + 0.02 * rs[m].random(n) for m in range(B)])
    uhat = np.stack([0.9 * u[m] + 0.02 * rs[m].random(tl) for m in range(B)])
    vhat = np.stack([1.1 * v[m] + 0.02 * rs[m].random(tl) for m in range(B)])

    def o_adj(m, optim, th_u, th_v):
        po, qo = np.zeros(tl), np.zeros(tl)
        return otraj.solve_adjoint_schnak_system(mem.to_dof(u[m]), mem.to_dof(v[m]), mem.to_dof(th_u[m]),
                                                 mem.to_dof(th_v[m]), po, qo, Nt * dt, asm, n, Nt, dt, None, optim)

    for optim, th_u, th_v in (("finaltime", uhat_T, vhat_T), ("alltime", uhat, vhat)):
        pq = _compare(f"pq_{optim}", D, mem,
                      lambda u_, v_, tu, tv, p_, q_, b, at=optim == "alltime":
                      ctx.schnak_adjoint(AwT, u_, v_, tu, tv, p_, q_, Nt, dt, par, batch=b, alltime=at),
                      [np.zeros((B, tl)), np.zeros((B, tl))], [u, v, th_u, th_v],
                      lambda m, o=optim, a=th_u, b_=th_v: o_adj(m, o, a, b_), ADJ_TOL, errs)
        assert np.abs(pq[0][:, :Nt * n]).max() > 0 and np.abs(pq[1][:, :Nt * n]).max() > 0
    return errs


def _chtxs(hp, systems, S, D, mem, N, dt):
    from oracle import traj as otraj
    _, asm = _oracle(N)
    ctx, n, Nt, tl, B = S.ctx, mem.n, mem.Nt, mem.tl, mem.B
    cpar = systems._chtxs_par()
    u0 = [1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs]
    v0 = [1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs]
    c = np.stack([20 * r.random(tl) for r in mem.rngs])
    errs = {}

    def o_fwd(m, per_step):
        def f():
            uo, vo = np.zeros(tl), np.zeros(tl)
            uo[:n], vo[:n] = mem.to_dof(u0[m]), mem.to_dof(v0[m])
            (pso if per_step else otraj).solve_chtxs_system(mem.to_dof(c[m]), uo, vo, asm, n, Nt, dt)
            return [uo, vo]
        return _cached(("chtxs", N, m, "ct" if per_step else "frozen"), f)

    u, v = _compare("uv", D, mem, lambda c_, u_, v_, b: ctx.chtxs_forward(c_, u_, v_, Nt, dt, cpar, 0.1, batch=b),
                    [mem.traj(u0), mem.traj(v0)], [c[:, n:2 * n]], lambda m: o_fwd(m, False), STATE_TOL, errs)
    _compare("uv_ct", D, mem, lambda c_, u_, v_, b: ctx.chtxs_forward_ct(c_, u_, v_, Nt, dt, cpar, 0.1, batch=b),
             [mem.traj(u0), mem.traj(v0)], [c], lambda m: o_fwd(m, True), STATE_TOL, errs)
    rs = mem.rngs
    uhat_T = np.stack([0.9 * u[m, Nt * n:] + 0.02 * rs[m].random(n) for m in range(B)])
    vhat_T = np.stack([1.05 * v[m, Nt * n:] + 0.02 * rs[m].random(n) for m in range(B)])
    uhat = np.stack([0.9 * u[m] + 0.02 * rs[m].random(tl) for m in range(B)])
    vhat = np.stack([1.05 * v[m] + 0.02 * rs[m].random(tl) for m in range(B)])

    def o_adj(m, optim, th_u, th_v):
        po, qo = np.zeros(tl), np.zeros(tl)
        return otraj.solve_adjoint_chtxs_system(mem.to_dof(u[m]), mem.to_dof(v[m]), mem.to_dof(th_u[m]), mem.to_dof(th_v[m]),
                                                po, qo, mem.to_dof(c[m]), Nt * dt, asm, n, Nt, dt, None, optim)

    for optim, th_u, th_v in (("finaltime", uhat_T, vhat_T), ("alltime", uhat, vhat)):
        pq = _compare(f"pq_{optim}", D, mem,
                      lambda u_, v_, tu, tv, c_, p_, q_, b, at=optim == "alltime":
                      ctx.chtxs_adjoint(u_, v_, tu, tv, p_, q_, c_, Nt, dt, cpar, 0.1, alltime=at, batch=b),
                      [np.zeros((B, tl)), np.zeros((B, tl))], [u, v, th_u, th_v, c],
                      lambda m, o=optim, a=th_u, b_=th_v: o_adj(m, o, a, b_), ADJ_TOL, errs)
        assert np.abs(pq[0][:, :Nt * n]).max() > 0 and np.abs(pq[1][:, :Nt * n]).max() > 0
    return errs


SYSTEMS = {"nonlinear": _nonlinear, "schnak": _schnak, "chtxs": _chtxs}


@pytest.mark.parametrize("system", list(SYSTEMS))
@pytest.mark.parametrize("N, B, regime, env", CASES)
def test_system_sweeps_vs_oracle(hp, systems, monkeypatch, N, B, regime, env, system):
    """Every sweep of ``system`` (forward with the frozen and the per-step control, the Schnakenberg one also with a
    time-dependent wind; adjoint with the final-time and the all-time misfit) on B members at once, in the kernel
    regime the case names: each member against the oracle (states < 1e-10, adjoints < 1e-9, relative l2) and against
    itself run alone (< 1e-12); no solve out of budget, every residual <= 1e-13, and every species solve on Chebyshev.
    The walkers case also checks that the Jacobi launches of the sweeps walked."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
    try:
        ctx = S.ctx
        knobs = _regime_knobs_default()
        if knobs:
            assert ctx.kernel_regime(B) == getattr(hp._lib, "REGIME_" + regime)
            if "FEMFCT_T4_WALKERS" in env:
                assert ctx.patch_walkers(B) == int(env["FEMFCT_T4_WALKERS"])
        Nt = _num_steps(N)
        mem = _Members(system, N, B, Nt)
        assert mem.n == ctx.n == N * N
        D = _Device(hp, ctx, Nt, species=system != "nonlinear", cheb=knobs)
        errs = SYSTEMS[system](hp, systems, S, D, mem, N, DT[system])
        if knobs and "FEMFCT_T4_WALKERS" in env:
            li = ctx.launch_info()               # the last sweep's Jacobi launch: persistent walkers, not one per patch
            assert li["jacobi_kernel"] in ("k_strip4_jacobi_walk", "k_strip_jacobi_pair_walk"), li
            assert li["jacobi_walkers"] > 0, li
        _report(f"{system} N={N} B={B} {regime}", **errs)
    finally:
        S.close()


@pytest.mark.parametrize("problem", ["schnak", "chtxs"])
def test_speculative_pgd_129x129_on_the_64_patch_kernels(hp, problem):
    """One projected-gradient iteration of the refactored drivers at 129 x 129 (vertex order, as the drop-in wrapper
    runs it) with six Armijo trials per launch: 6 x 16 641 nodes put every forward sweep of the line search on the
    64-patch kernels.  Against oracle.pdeco.projected_gradient_descent: the same Armijo decisions, every margin to 1e-6,
    costs to 1e-9, and the smallest |margin| far above the agreement of a cost evaluation.  Every sweep of the loop is
    checked as in the cases above: no solve out of budget, residuals <= 1e-13, every species solve on Chebyshev.
    The first trial step s0 is not the drivers' default (1 for Schnakenberg, 2 for chemotaxis): with it all six trials are
    rejected here, so s0 is set to where the line search rejects and then accepts."""
    from oracle import pdeco as opdeco, traj as otraj
    N, Nt, dt = 129, 10, 5e-4
    mesh, asm = _oracle(N)
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    n = V.nodes
    tl = (Nt + 1) * n
    z = lambda x0: np.concatenate([x0, np.zeros(Nt * n)])
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]       # DoF order
    if problem == "schnak":
        u0 = 1.0 + 0.1 * np.cos(2 * np.pi * (x + y))
        v0 = 0.9 + 0.1 * np.cos(2 * np.pi * (x - y))
        ut, vt = otraj.solve_schnak_system(np.full(tl, 0.1), z(u0), z(v0), asm, n, Nt, dt)
        targets = (ut[Nt * n:].copy(), vt[Nt * n:].copy())               # final-time misfit
    else:
        rng = np.random.default_rng(129)
        u0 = 1.5 + 0.1 * (0.5 - rng.random(n))
        v0 = u0.copy()
        ut, vt = otraj.solve_chtxs_system(np.full(tl, 10.0), z(u0), z(v0), asm, n, Nt, dt)
        targets = (ut.copy(), vt.copy())                                 # all-time misfit
    # oracle margins with these s0: schnak 49.9, 11.9, 1.03, -0.93; chtxs 0.337, -0.486
    opts = dict(max_iter_GD=1, max_iter_armijo=6, tol=0.0, s0=1 / 64 if problem == "schnak" else 0.05)
    ref = opdeco.projected_gradient_descent(problem, asm, asm.mass(), (u0, v0), targets, Nt, dt, **opts)
    mref = [m for ms in ref["armijo_margin"] for m in ms]
    with hp.SystemPDECO(problem, V, Nt, dt, **opts) as prob:
        knobs = _regime_knobs_default()
        if knobs:
            assert prob.ctx.kernel_regime(6) == hp._lib.REGIME_PATCH64
        ctx, sweeps = prob.ctx, []

        def checked(fn):
            def run(*args, batch=1, **kw):
                fn(*args, batch=batch, **kw)
                _check_logs(hp, ctx.traj_info(Nt, batch), False)
                _check_logs(hp, ctx.traj_krylov_info(Nt, batch), knobs)
                sweeps.append(batch)
            return run
        for name in (f"{problem}_forward", f"{problem}_adjoint"):
            setattr(ctx, name, checked(getattr(ctx, name)))
        got = prob.run((u0, v0), targets, speculative=True)
        assert 6 in sweeps, sweeps
    assert got["it"] == ref["it"] and got["restored"] == ref["restored"] and not ref["restored"]
    assert got["armijo_its"] == ref["armijo_its"], (got["armijo_its"], ref["armijo_its"])
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9)
    mgot = [m for ms in got["armijo_margin"] for m in ms]
    assert len(mgot) == len(mref) >= 2
    np.testing.assert_allclose(mgot, mref, rtol=1e-6)
    errs = {k: rel(got[k], ref[k]) for k in ("c", "u", "v", "p", "q")}
    _report(f"{problem} PGD 129^2 x {Nt} steps, 6 trials: armijo_its {got['armijo_its']}, smallest |margin| "
            f"{min(abs(m) for m in mref):.2e}", **errs)
    assert min(abs(m) for m in mref) > 1e-9
