"""The chemotaxis sweeps with a cell-growth term r(u) = u (r0 + r1 u + r2 u^2) on the device (-m gpu), against the CPU
reference tests/chtxs_growth_oracle.py, in every kernel regime.  Set-up, tolerances and the log checks are those of
tests/test_gpu_systems_regimes.py (its helpers are used as they are): per-member random initial states
1.5 + 0.1 (0.5 - rand) and controls 20 rand, dt = 5e-4, 4 steps; states to 1e-10, adjoints to 1e-9, a member against
itself run alone to 1e-12; no solve out of budget, residuals <= 1e-13."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import chtxs_growth_oracle as go
import test_gpu_systems_regimes as reg
from test_chtxs_growth_oracle import closed_form

pytestmark = pytest.mark.gpu

MIMURA, LOGISTIC = (0.0, 1.0, -1.0), (4.0, -1.0, 0.0)
STATE_TOL, ADJ_TOL = reg.STATE_TOL, reg.ADJ_TOL
DT, NT = 5e-4, 4
rel = reg.rel

# PGD test: the drivers' first trial step s0 = 2 is rejected six times here; 0.8 is where the search of the reference
# rejects and then accepts in both iterations.  Its margins (> 0: rejected): 1.556, -0.330; 0.476, 0.145, -0.0105
PGD_OPTS = dict(max_iter_GD=2, max_iter_armijo=6, tol=0.0, s0=0.8)

# nodes per side and batch: the smallest that reach each regime
CASES = [
    pytest.param(21, 1, "fenics", ("ROWS", "STRIPS"), [MIMURA], id="N21-B1-fenics-order"),
    pytest.param(41, 1, "vertex", ("MESH",), [MIMURA], id="N41-B1-one-workgroup"),
    pytest.param(41, 8, "vertex", ("MESH",), [MIMURA], id="N41-B8-one-workgroup"),
    pytest.param(46, 1, "vertex", ("TILE32",), [MIMURA, LOGISTIC], id="N46-B1-tile-cheb"),
    pytest.param(47, 8, "vertex", ("TILE32",), [MIMURA], id="N47-B8-single-patch"),
    pytest.param(61, 5, "vertex", ("TILE32",), [MIMURA], id="N61-B5"),
    pytest.param(81, 14, "vertex", ("PATCH64",), [MIMURA], id="N81-B14-patch64"),
]


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def systems():
    return importlib.import_module("fem-fct-pdeco_amd.systems")


def _members(N, B, order):
    mem = reg._Members("chtxs", N, B, NT)
    if order == "fenics":                      # the device works in DoF order: nothing to permute
        mem.v2d = np.arange(mem.n)
    return mem


def _data(mem):
    n, tl = mem.n, mem.tl
    u0 = [1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs]
    v0 = [1.5 + 0.1 * (0.5 - r.random(n)) for r in mem.rngs]
    c = np.stack([20 * r.random(tl) for r in mem.rngs])
    return u0, v0, c


def _growth_sweeps(S, D, mem, N, order, growth, cpar):
    """Forward (frozen and per-step control) and adjoint (final-time, all-time) with ``growth`` against the CPU reference,
    then against the device's growth-free sweeps, from which they must differ."""
    _, asm = reg._oracle(N)
    ctx, n, tl, B = S.ctx, mem.n, mem.tl, mem.B
    u0, v0, c = _data(mem)
    errs = {}

    def o_fwd(m, per_step):
        def f():
            uo, vo = np.zeros(tl), np.zeros(tl)
            uo[:n], vo[:n] = mem.to_dof(u0[m]), mem.to_dof(v0[m])
            go.solve_chtxs_system(mem.to_dof(c[m]), uo, vo, asm, n, NT, DT, growth=growth, per_step=per_step)
            return [uo, vo]
        return reg._cached(("chtxs_growth", N, order, m, growth, per_step), f)

    ins = [mem.traj(u0), mem.traj(v0)]
    u, v = reg._compare("uv", D, mem, lambda c_, u_, v_, b: ctx.chtxs_forward(c_, u_, v_, NT, DT, cpar, 0.1, batch=b, growth=growth),
                        ins, [c[:, n:2 * n]], lambda m: o_fwd(m, False), STATE_TOL, errs)
    reg._compare("uv_ct", D, mem, lambda c_, u_, v_, b: ctx.chtxs_forward_ct(c_, u_, v_, NT, DT, cpar, 0.1, batch=b, growth=growth),
                 ins, [c], lambda m: o_fwd(m, True), STATE_TOL, errs)
    rs = mem.rngs
    uhat = np.stack([0.9 * u[m] + 0.02 * rs[m].random(tl) for m in range(B)])
    vhat = np.stack([1.05 * v[m] + 0.02 * rs[m].random(tl) for m in range(B)])

    def o_adj(m, optim, tu, tv):
        return go.solve_adjoint_chtxs_system(mem.to_dof(u[m]), mem.to_dof(v[m]), mem.to_dof(tu[m]), mem.to_dof(tv[m]),
                                             np.zeros(tl), np.zeros(tl), mem.to_dof(c[m]), NT * DT, asm, n, NT, DT, None,
                                             optim, growth=growth)

    zeros = [np.zeros((B, tl)), np.zeros((B, tl))]
    p = {}
    for optim, tu, tv in (("finaltime", uhat[:, NT * n:], vhat[:, NT * n:]), ("alltime", uhat, vhat)):
        adj = lambda g: (lambda u_, v_, a_, b_, c_, p_, q_, b, at=optim == "alltime":
                         ctx.chtxs_adjoint(u_, v_, a_, b_, p_, q_, c_, NT, DT, cpar, 0.1, alltime=at, batch=b, growth=g))
        p[optim] = reg._compare(f"pq_{optim}", D, mem, adj(growth), zeros, [u, v, tu, tv, c],
                                lambda m, o=optim, a=tu, b_=tv: o_adj(m, o, a, b_), ADJ_TOL, errs)[0]
        p_free = D.run(adj(None), zeros, [u, v, tu, tv, c], B)[0]
        # r'(1.5) = -3.75 (m^2 (1 - m)) over 2e-3 time units: about 7e-3 expected; an ignored keyword gives 0
        errs[f"p_{optim}_moved"] = rel(p[optim][:, :NT * n], p_free[:, :NT * n])
        assert errs[f"p_{optim}_moved"] > 1e-4, errs
    u_free = D.run(lambda c_, u_, v_, b: ctx.chtxs_forward(c_, u_, v_, NT, DT, cpar, 0.1, batch=b), ins, [c[:, n:2 * n]], B)[0]
    errs["u_moved"] = rel(u[:, n:], u_free[:, n:])      # r(1.5) = -1.125 over 2e-3 time units: about 2e-3 expected
    assert errs["u_moved"] > 1e-4, errs
    return errs


@pytest.mark.parametrize("N, B, order, regimes, growths", CASES)
def test_growth_sweeps_vs_reference(hp, systems, N, B, order, regimes, growths):
    """Every chemotaxis sweep with growth on B members in the kernel regime the case names: each member against the CPU
    reference and against itself run alone, both solver logs clean, and the answers moved by growth (> 1e-4 relative l2
    in u and in p against the device's growth-free sweeps), so that a silently ignored keyword cannot pass."""
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    S = systems.PDESystems(V, order=hp.ORDER_FENICS if order == "fenics" else hp.ORDER_VERTEX)
    try:
        knobs = reg._regime_knobs_default()
        if knobs:
            assert S.ctx.kernel_regime(B) in [getattr(hp._lib, "REGIME_" + r) for r in regimes]
        mem = _members(N, B, order)
        assert mem.n == S.ctx.n == N * N
        D = reg._Device(hp, S.ctx, NT, species=True, cheb=knobs and order == "vertex")
        for growth in growths:
            errs = _growth_sweeps(S, D, mem, N, order, growth, systems._chtxs_par())
            reg._report(f"chtxs growth {growth} N={N} B={B} {order} {'/'.join(regimes)}", **errs)
    finally:
        S.close()


def _run(ctx, n, B, u0, v0, c, growth, Nt=NT, dt=DT, cpar=None, per_step=False, adjoint=None):
    """one forward sweep (and, with adjoint=(uhat, vhat, alltime), one adjoint sweep) on fresh device buffers"""
    tl = (Nt + 1) * n
    tr = lambda x0: np.concatenate([np.concatenate([x, np.zeros(Nt * n)]) for x in x0])
    bufs = [ctx.array(tr(u0)), ctx.array(tr(v0)), ctx.array(np.ascontiguousarray(c).ravel())]
    try:
        u, v, cd = bufs
        if per_step:
            ctx.chtxs_forward_ct(cd, u, v, Nt, dt, cpar, 0.1, batch=B, growth=growth)
        else:
            ctx.chtxs_forward(cd, u, v, Nt, dt, cpar, 0.1, batch=B, growth=growth)
        out = [u.download(), v.download()]
        if adjoint is not None:
            uhat, vhat, alltime = adjoint
            ct = c if per_step else np.tile(np.asarray(c).reshape(B, 1, n), (1, Nt + 1, 1))
            bufs += [ctx.array(np.ascontiguousarray(a).ravel()) for a in (uhat, vhat, ct)] + [ctx.zeros(B * tl), ctx.zeros(B * tl)]
            ctx.chtxs_adjoint(u, v, bufs[3], bufs[4], bufs[6], bufs[7], bufs[5], Nt, dt, cpar, 0.1, alltime=alltime, batch=B,
                              growth=growth)
            out += [bufs[6].download(), bufs[7].download()]
        return out
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("N, B", [(41, 8), (81, 14)])
def test_zero_growth_is_no_growth_bit_for_bit(hp, systems, N, B):
    """growth=(0, 0, 0) equals growth=None bit for bit on the device, forward and (all-time) adjoint.  Each on a context of
    its own: a context's second sweep of a kind runs with the budgets its first one settled, so that two sweeps in a row
    on one context agree to the solver tolerance, not in their bits, growth or not."""
    n = N * N
    rng = np.random.default_rng([N, B])
    u0 = [1.5 + 0.1 * (0.5 - rng.random(n)) for _ in range(B)]
    v0 = [1.5 + 0.1 * (0.5 - rng.random(n)) for _ in range(B)]
    c = 20 * rng.random((B, n))
    tl = (NT + 1) * n
    uhat, vhat = 1.4 + 0.1 * rng.random((B, tl)), 1.6 + 0.1 * rng.random((B, tl))
    out = []
    for growth in (None, (0.0, 0.0, 0.0)):
        S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, N - 1), order=hp.ORDER_VERTEX)
        try:
            out.append(_run(S.ctx, n, B, u0, v0, c, growth, cpar=systems._chtxs_par(), adjoint=(uhat, vhat, True)))
        finally:
            S.close()
    assert np.abs(out[0][2]).max() > 0
    for x, y in zip(*out):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("N", [41, 46])
def test_graphs_carry_the_coefficients(hp, systems, N):
    """With growth, graph replay and kernel-by-kernel enqueue give the same bits; and two coefficient sets in turn on one
    context (same buffers' addresses or not, budgets settled) give what fresh contexts give: the graph keys carry the
    coefficients."""
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    cpar = systems._chtxs_par()
    rng = np.random.default_rng(N)
    n = N * N
    u0, v0 = [1.5 + 0.1 * (0.5 - rng.random(n))], [1.5 + 0.1 * (0.5 - rng.random(n))]
    c = 20 * rng.random((1, n))
    tl = (NT + 1) * n
    adj = (1.4 + 0.1 * rng.random((1, tl)), 1.6 + 0.1 * rng.random((1, tl)), True)
    run = lambda ctx, g: _run(ctx, n, 1, u0, v0, c, g, cpar=cpar, adjoint=adj)
    fresh = {}
    for g in (MIMURA, LOGISTIC):
        S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
        try:
            fresh[g] = run(S.ctx, g)
            if S.ctx.graph_replay_active():
                again = run(S.ctx, g)                       # budgets settled: the sweep the comparison below replays
                S.ctx.set_graphs(False)
                plain = run(S.ctx, g)
                for x, y in zip(again, plain):
                    assert np.array_equal(x, y)
        finally:
            S.close()
    assert rel(fresh[MIMURA][0], fresh[LOGISTIC][0]) > 1e-4
    S = systems.PDESystems(V, order=hp.ORDER_VERTEX)
    try:
        for g in (MIMURA, MIMURA, LOGISTIC, LOGISTIC, MIMURA):
            got = run(S.ctx, g)
            for k, (x, y) in enumerate(zip(got, fresh[g])):
                assert rel(x, y) < (STATE_TOL if k < 2 else ADJ_TOL), (g, k, rel(x, y))
    finally:
        S.close()


@pytest.mark.parametrize("growth", [MIMURA, LOGISTIC], ids=["m2(1-m)", "m(4-m)"])
def test_constant_states_closed_form_on_the_device(hp, systems, growth):
    """u = a, v = b, constant control and constant terminal values at 41 x 41: forward and final-time adjoint equal the
    scalar recursions (test_chtxs_growth_oracle.closed_form) to 1e-12.  The device's solves stop at a relative residual,
    1e-13 by default: times the condition number of the species matrix (about 24: the P1 mass matrix with its lighter
    boundary rows) and six steps that does not promise 1e-12 (measured with it: u 3.1e-13, v 2.2e-13, p 1.8e-12, q 1.2e-12),
    so both solvers are asked for 1e-14 here."""
    N, Nt, dt, resc = 41, 6, 5e-3, 0.1
    S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, N - 1), order=hp.ORDER_VERTEX)
    try:
        S.ctx.set_solver(rel_tol=1e-14)
        S.ctx.set_krylov(rel_tol=1e-14)
        n = S.ctx.n
        a0, b0, cc, pT, qT = 1.5, 1.2, 7.0, 0.3, -0.2
        cpar = systems._chtxs_par()
        u, v = _run(S.ctx, n, 1, [np.full(n, a0)], [np.full(n, b0)], np.full((1, (Nt + 1) * n), cc), growth, Nt=Nt, dt=dt,
                    cpar=cpar, per_step=True)
        uhat, vhat = np.full((1, n), u[Nt * n] + pT), np.full((1, n), v[Nt * n] + qT)
        _, _, p, q = _run(S.ctx, n, 1, [np.full(n, a0)], [np.full(n, b0)], np.full((1, (Nt + 1) * n), cc), growth, Nt=Nt,
                          dt=dt, cpar=cpar, per_step=True, adjoint=(uhat, vhat, False))
        a, b, ps, qs = closed_form(growth, a0, b0, cc, pT, qT, Nt, dt, cpar[0], resc)
        err = lambda x, s: np.abs(x.reshape(Nt + 1, n) - s[:, None]).max() / np.abs(s).max()
        errs = dict(u=err(u, a), v=err(v, b), p=err(p, ps), q=err(q, qs))
        reg._report(f"chtxs growth {growth} closed form N={N}", **errs)
        assert max(errs.values()) < 1e-12, errs
    finally:
        S.close()


def test_invalid_growth(hp, systems):
    """A coefficient that is not finite is a ValueError at entry; NaN in u0 with growth fails the solve (NotConverged)."""
    N = 21
    S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, N - 1), order=hp.ORDER_VERTEX)
    try:
        n, cpar = S.ctx.n, systems._chtxs_par()
        u0, c = np.full(n, 1.5), np.full((1, n), 5.0)
        for bad in ((np.nan, 1.0, -1.0), (0.0, np.inf, -1.0)):
            with pytest.raises(ValueError):
                _run(S.ctx, n, 1, [u0], [u0], c, bad, cpar=cpar)
        with pytest.raises(ValueError):
            _run(S.ctx, n, 1, [u0], [u0], c, (1.0, 2.0), cpar=cpar)
        with pytest.raises(ValueError):
            hp.SystemPDECO("schnak", hp.SquareMeshP1(0.0, 1.0, N - 1), 2, DT, growth=MIMURA)
        un = u0.copy()
        un[n // 2] = np.nan
        with pytest.raises(hp._lib.NotConverged):
            _run(S.ctx, n, 1, [un], [u0], c, MIMURA, cpar=cpar)
    finally:
        S.close()


@pytest.mark.parametrize("speculative", [True, False], ids=["speculative", "sequential"])
def test_pgd_with_growth_vs_reference(hp, speculative):
    """SystemPDECO("chtxs", growth=(0, 1, -1), control_per_step=True) at 41 x 41, 10 steps, two iterations, against
    oracle.pdeco.projected_gradient_descent with the chemotaxis sweeps replaced by the growth reference: the same Armijo
    decisions, costs to 1e-9, margins to 1e-6, final c, u, v, p, q to 1e-7, and the smallest |margin| above 1e-9."""
    from oracle import pdeco as opdeco
    N, Nt, dt = 41, 10, 5e-4
    mesh, asm = reg._oracle(N)
    V = hp.SquareMeshP1(0.0, 1.0, N - 1)
    n = V.nodes
    tl = (Nt + 1) * n
    z = lambda x0: np.concatenate([x0, np.zeros(Nt * n)])
    rng = np.random.default_rng(41)
    u0 = 1.5 + 0.1 * (0.5 - rng.random(n))
    v0 = u0.copy()

    def reference():
        ut, vt = go.solve_chtxs_system(np.full(tl, 10.0), z(u0), z(v0), asm, n, Nt, dt, growth=MIMURA, per_step=True)
        targets = (ut.copy(), vt.copy())
        with go.patched(MIMURA, True):
            return targets, opdeco.projected_gradient_descent("chtxs", asm, asm.mass(), (u0, v0), targets, Nt, dt, **PGD_OPTS)
    targets, ref = reg._cached(("chtxs_growth_pgd", N), reference)
    mref = [m for ms in ref["armijo_margin"] for m in ms]
    got = hp.projected_gradient_descent("chtxs", V, (u0, v0), targets, Nt, dt, speculative=speculative,
                                        control_per_step=True, growth=MIMURA, **PGD_OPTS)
    assert got["it"] == ref["it"] == 2 and got["restored"] == ref["restored"] and not ref["restored"]
    assert got["armijo_its"] == ref["armijo_its"], (got["armijo_its"], ref["armijo_its"])
    assert max(ref["armijo_its"]) >= 2 and max(ref["armijo_its"]) < PGD_OPTS["max_iter_armijo"]    # rejects, then accepts
    mgot = [m for ms in got["armijo_margin"] for m in ms]
    errs = {k: rel(got[k], ref[k]) for k in ("c", "u", "v", "p", "q")}
    reg._report(f"chtxs growth PGD 41^2 x {Nt} steps, {'speculative' if speculative else 'sequential'}: armijo_its "
                f"{got['armijo_its']}, margins {['%.3g' % m for m in mref]}", **errs)
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9)
    assert len(mgot) == len(mref)
    np.testing.assert_allclose(mgot, mref, rtol=1e-6)
    assert max(errs.values()) < 1e-7, errs
    assert min(abs(m) for m in mref) > 1e-9


def test_example_runs_at_a_reduced_size():
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "chemotaxis_growth_pdeco.py"), "--nodes", "21", "--pattern-steps",
                          "20", "--steps", "10", "--iters", "2"], capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "pattern run: 20 steps" in out.stdout and "chtxs with growth (alltime): 2 PGD iterations in" in out.stdout
