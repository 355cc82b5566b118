"""Smooth controls on the device (-m gpu): the kernels of kernels_smooth.hip against the NumPy reference of
smoothness_oracle.py, the fused right-hand side against its two parts bit for bit, the loops against the CPU loops, the
composition with control intervals, error paths and the example.

Device data is in the context's DoF order (FEniCS or vertex order), the oracle's in FEniCS DoF order; ``_Order`` converts.
The CPU loops and their inputs are those of test_smoothness_oracle.py (computed once per process)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import smoothness_oracle as smo
from test_gpu_snapshots import ADJ_TOL, EPS, OM, _Order, _fields, _oracle, rel
from test_gpu_state_bounds import pgd_case  # noqa: F401  (the fixture of the state-bounds loop tests)
from test_smoothness_oracle import PGD_ROWS, SOURCE_COEFFS, cpu_pgd, cpu_source, rough_start, source_inputs

pytestmark = pytest.mark.gpu

# femfct_geom gives one block of 64 threads per 64 rows while n <= 65536 (kernels_step.hip): 9 x 9 = 81 nodes is the
# smallest square mesh with more than one block in x (8 x 8 = 64 has one)
N_TWO_BLOCKS = 9
COEFFS = [(0.7, 0.0), (0.0, 3e-6), (0.7, 3e-6)]


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _problem(hp, solvers, N, Nt, dt, vertex, batch=1):
    return solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, N - 1), Nt, dt, om=OM, batch=batch,
                                  order=hp.ORDER_VERTEX if vertex else hp.ORDER_FENICS)


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("Nt", [1, 2, 5])
@pytest.mark.parametrize("N", [5, N_TWO_BLOCKS, 21])
def test_smooth_rhs_and_cost_kernels(hp, solvers, N, Nt, vertex):
    """femfct_smooth_rhs and femfct_smooth_cost against NumPy, batch 1 and 3, the coefficient pairs (beta_x, 0),
    (0, beta_t) and both.  smooth_rhs: row i within 64 eps A_i, A_i the row's sum of term magnitudes
    beta_x |Ad| |c| + beta_t |M| (2 |c_l| + |c_{l-1}| + |c_{l+1}|) / dt^2 (fewer than 32 rounded operations touch any
    term).  smooth_cost: within m eps S_abs, m the number of products summed and S_abs the sum of their magnitudes, the
    worst case of any summation order (wrong end weights or end levels are O(1 / levels)).  Every call is repeated and
    returns the same bits; a member of the batch and the member alone: the same bits.  Nt = 1: both levels are end
    levels."""
    mesh, asm = _oracle(N)
    M, Ad = asm.mass(), asm.stiffness()
    od = _Order(mesh, vertex)
    n, dt = mesh.nodes, 2.5e-3
    tl = (Nt + 1) * n
    prob = _problem(hp, solvers, N, Nt, dt, vertex, batch=3)
    ctx = prob.ctx
    worst_r = worst_c = 0.0
    try:
        for B in (1, 3):
            c = _fields(mesh, B * (Nt + 1), [N, Nt, B]).reshape(B, tl)
            dc, out = ctx.array(od.to_dev(c.reshape(-1, n)).ravel()), ctx.zeros(B * tl)
            for bx, bt in COEFFS:
                ctx.smooth_rhs(dc, bx, bt, Nt, dt, out, batch=B)
                got = out.download()
                ctx.smooth_rhs(dc, bx, bt, Nt, dt, out.zero(), batch=B)
                assert np.array_equal(bits(out.download()), bits(got))
                for m in range(B):
                    ref = smo.smooth_rhs(M, Ad, c[m], Nt, dt, bx, bt)
                    A = smo.rhs_magnitude(M, Ad, c[m], Nt, dt, bx, bt)
                    err = np.abs(od.from_dev(got[m * tl:(m + 1) * tl]) - ref)
                    assert ref.any() and np.all(err <= 64 * EPS * A), (B, bx, bt, m, (err / A).max() / EPS)
                    worst_r = max(worst_r, (err / A).max() / EPS)
                    if B > 1:
                        one = ctx.zeros(tl)
                        ctx.smooth_rhs(dc.ptr + 8 * m * tl, bx, bt, Nt, dt, one, batch=1)
                        assert np.array_equal(bits(one.download()), bits(got[m * tl:(m + 1) * tl]))
            S = ctx.smooth_cost(dc, Nt, dt, batch=B)
            assert S.shape == (B, 2) and np.array_equal(bits(ctx.smooth_cost(dc, Nt, dt, batch=B)), bits(S))
            for m in range(B):
                Rx, Rt = smo.roughness(M, Ad, c[m], Nt, dt)
                Sx, St, mx, mt = smo.cost_magnitude(M, Ad, c[m], Nt, dt)
                print(f"[smoothness] cost N={N} Nt={Nt} B={B} m={m}: R_x {S[m, 0]:.15e} (CPU {Rx:.15e}), "
                      f"R_t {S[m, 1]:.15e} (CPU {Rt:.15e})")
                assert abs(S[m, 0] - Rx) <= mx * EPS * Sx and abs(S[m, 1] - Rt) <= mt * EPS * St
                assert Rx > 0 and Rt > 0
                worst_c = max(worst_c, abs(S[m, 0] - Rx) / (EPS * Sx), abs(S[m, 1] - Rt) / (EPS * St))
                assert np.array_equal(bits(ctx.smooth_cost(dc.ptr + 8 * m * tl, Nt, dt, batch=1)[0]), bits(S[m]))
        print(f"[smoothness] N={N} Nt={Nt}: worst smooth_rhs row error {worst_r:.2f} eps A_i (bound 64), worst smooth_cost "
              f"error {worst_c:.2f} eps S_abs")
    finally:
        prob.close()


def test_zero_coefficients_read_nothing_else(hp, solvers):
    """beta_t = 0: no neighbouring level is read, so a NaN level leaves the other levels' rows as they are, bit for bit;
    both zero: zeros."""
    N, Nt, dt = N_TWO_BLOCKS, 3, 2.5e-3
    mesh, _ = _oracle(N)
    n = mesh.nodes
    tl = (Nt + 1) * n
    c = _fields(mesh, Nt + 1, [N, 77]).ravel()
    holes = c.copy()
    holes[n:2 * n] = np.nan
    prob = _problem(hp, solvers, N, Nt, dt, True)
    ctx = prob.ctx
    try:
        out = ctx.zeros(tl)
        ctx.smooth_rhs(ctx.array(c), 0.7, 0.0, Nt, dt, out)
        full = out.download()
        ctx.smooth_rhs(ctx.array(holes), 0.7, 0.0, Nt, dt, out.zero())
        got = out.download()
        assert np.isnan(got[n:2 * n]).all() and full.any()
        assert np.array_equal(bits(got[:n]), bits(full[:n])) and np.array_equal(bits(got[2 * n:]), bits(full[2 * n:]))
        ctx.smooth_rhs(ctx.array(c), 0.0, 0.0, Nt, dt, out)
        assert not out.download().any()
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ fusion
@pytest.mark.parametrize("vertex", [False, True], ids=["fenics", "vertex"])
@pytest.mark.parametrize("N, Nt", [(N_TWO_BLOCKS, 1), (21, 5)])
def test_fused_rhs_equals_its_parts_bitwise(hp, solvers, N, Nt, vertex):
    """femfct_drift_gradient_rhs_smooth = femfct_drift_gradient_rhs + femfct_smooth_rhs (added by femfct_axpby(1, ., 1, .))
    bit for bit, for the three coefficient pairs; with zero coefficients femfct_drift_gradient_rhs bit for bit."""
    mesh, _ = _oracle(N)
    n, dt, beta = mesh.nodes, 2.5e-3, 0.05
    tl = (Nt + 1) * n
    c, u, p = (_fields(mesh, Nt + 1, [N, Nt, k]).ravel() for k in range(3))
    prob = _problem(hp, solvers, N, Nt, dt, vertex)
    ctx = prob.ctx
    try:
        dc, du, dp = ctx.array(c), ctx.array(u), ctx.array(p)
        a, b, s, f = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl)
        ctx.drift_gradient_rhs(dc, du, dp, beta, a, Nt + 1, prob.drift)
        drift = a.download()
        for bx, bt in COEFFS:
            ctx.smooth_rhs(dc, bx, bt, Nt, dt, b)
            ctx.axpby(tl, 1.0, a, 1.0, b, s)
            ctx.drift_gradient_rhs_smooth(dc, du, dp, beta, bx, bt, dt, f.zero(), Nt + 1, prob.drift)
            got, want = f.download(), s.download()
            assert np.array_equal(bits(got), bits(want)) and not np.array_equal(got, drift), (bx, bt)
        ctx.drift_gradient_rhs_smooth(dc, du, dp, beta, 0.0, 0.0, dt, f.zero(), Nt + 1, prob.drift)
        assert np.array_equal(bits(f.download()), bits(drift)) and drift.any()
    finally:
        prob.close()


def test_cost_with_zero_coefficients_is_the_cost_bitwise(hp, solvers):
    """prob.cost(..., smoothness=Smoothness(0, 0)) equals the cost without the keyword bit for bit in every mode, batch 2,
    and keeps (R_x, R_t) of the pass; with coefficients it adds beta_x/2 R_x + beta_t/2 R_t."""
    N, Nt, dt, B = 21, 5, 2.5e-3, 2
    mesh, asm = _oracle(N)
    n = mesh.nodes
    tl = (Nt + 1) * n
    u, uh, c = (_fields(mesh, B * (Nt + 1), [N, 9, k]).ravel() for k in range(3))
    uhT = np.concatenate([uh[b * tl + Nt * n:(b + 1) * tl] for b in range(B)])
    prob = _problem(hp, solvers, N, Nt, dt, False, batch=B)
    ctx = prob.ctx
    try:
        du, dh, dhT, dc = ctx.array(u), ctx.array(uh), ctx.array(uhT), ctx.array(c)
        for optim, tgt, obs in (("finaltime", dhT, None), ("alltime", dh, None),
                                ("snapshots", dh, solvers.Observations(Nt, [2, Nt], [0.7, 1.3]))):
            J0 = prob.cost(du, tgt, dc, 0.05, optim, batch=B, obs=obs)
            J1 = prob.cost(du, tgt, dc, 0.05, optim, batch=B, obs=obs, smoothness=solvers.Smoothness(0, 0))
            assert np.array_equal(bits(J1), bits(J0)) and J0.all(), optim
            st = prob.last_smooth_stats.copy()
            J2 = prob.cost(du, tgt, dc, 0.05, optim, batch=B, obs=obs, smoothness=solvers.Smoothness(0.3, 2e-6))
            assert np.array_equal(J2, J0 + (0.3 / 2 * st[:, 0] + 2e-6 / 2 * st[:, 1])) and np.all(J2 > J0)
            assert np.array_equal(bits(st), bits(ctx.smooth_cost(dc, Nt, dt, batch=B))) and np.all(st > 0)
    finally:
        prob.close()


# ------------------------------------------------------------------------------------------------ the loops
def _close(a, b):
    return np.all(np.abs(np.array(a) - np.array(b)) <= 1e-10 * np.abs(np.array(b)))


def _compare_histories(h, ho):
    assert h["armijo_k"] == ho["armijo_k"], (h["armijo_k"], ho["armijo_k"])
    assert _close(h["cost"], ho["cost"]), (h["cost"], ho["cost"])
    assert _close(h["roughness_x"], ho["roughness_x"]), (h["roughness_x"], ho["roughness_x"])
    assert _close(h["roughness_t"], ho["roughness_t"]), (h["roughness_t"], ho["roughness_t"])


def _device_pgd(hp, solvers, k, optim, sm):
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    od = _Order(k["mesh"], True)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    try:
        target = od.to_dev(k["tgt"][Nt * n:]) if optim == "finaltime" else od.to_dev(k["tgt"])
        u, p, c, h = solvers.pgd_solidbody(prob, od.to_dev(k["u0"]), target, od.to_dev(rough_start(k)), k["beta"], 0.0, 5.0,
                                           4, max_armijo=8, optim=optim, smoothness=sm)
    finally:
        prob.close()
    return od.from_dev(u), od.from_dev(c), h


@pytest.mark.parametrize("optim, bx, bt, trials", PGD_ROWS)
def test_pgd_solidbody_matches_the_cpu_loop(hp, solvers, pgd_case, optim, bx, bt, trials):
    """pgd_solidbody(smoothness=...) against the CPU loop on pgd_case (N = 21, 20 steps, dt = 2e-3, beta = 0.05, control
    bounds 0..5) from the start control 0.5 + 0.3 sin(6x) cos(5y) cos(400t), 4 iterations, max_armijo = 8: equal Armijo
    trial counts, costs and both roughness histories to 1e-10 relative, state and control to ADJ_TOL; the CPU loop's
    smallest Armijo margin is >= 1e-8 (asserted).  Measured on the CPU: final-time (7e-4, 0): trials [1, 1, 1, 3],
    smallest margin 9.2e-4; final-time (6e-4, 1.2e-6): [1, 1, 1, 2], 5.9e-5; all-time (0, 1.5e-6): [1, 1, 1, 2], 1.0e-2."""
    uo, po, co, ho = cpu_pgd(pgd_case, optim, bx, bt)
    assert ho["armijo_margin_min"] >= 1e-8 and ho["armijo_k"] == trials
    u, c, h = _device_pgd(hp, solvers, pgd_case, optim, solvers.Smoothness(bx, bt))
    print(f"[smoothness] PGD {optim} ({bx}, {bt}): device costs {h['cost']}, CPU {ho['cost']}; trials {h['armijo_k']}; "
          f"R_x {h['roughness_x']}, R_t {h['roughness_t']}; state {rel(u, uo):.2e}, control {rel(c, co):.2e}")
    _compare_histories(h, ho)
    assert rel(u, uo) < ADJ_TOL and rel(c, co) < ADJ_TOL


def test_pgd_solidbody_smooths_the_control(hp, solvers, pgd_case):
    """The point of the term, a fact of the CPU loop re-asserted on the device: final-time, after 4 iterations
    (0, 0) leaves R_t = 104.1, R_x = 0.289; (2e-4, 4e-7) gives R_t = 26.9, R_x = 0.211 (CPU smallest margin 3.3e-2)."""
    runs = []
    for bx, bt in ((0.0, 0.0), (2e-4, 4e-7)):
        *_, ho = cpu_pgd(pgd_case, "finaltime", bx, bt)
        assert ho["armijo_margin_min"] >= 1e-8
        u, c, h = _device_pgd(hp, solvers, pgd_case, "finaltime", solvers.Smoothness(bx, bt))
        _compare_histories(h, ho)
        runs.append(h)
    h0, h1 = runs
    print(f"[smoothness] after 4 iterations: R_t {h0['roughness_t'][-1]:.4f} -> {h1['roughness_t'][-1]:.4f}, "
          f"R_x {h0['roughness_x'][-1]:.5f} -> {h1['roughness_x'][-1]:.5f}")
    assert abs(h0["roughness_t"][-1] - 104.1) < 0.05 and abs(h1["roughness_t"][-1] - 26.9) < 0.05
    assert abs(h0["roughness_x"][-1] - 0.289) < 5e-4 and abs(h1["roughness_x"][-1] - 0.211) < 5e-4


def test_pgd_source_control_matches_the_cpu_loop(hp, solvers):
    """pgd_source_control(increment="resolve", smoothness=...), all-time tracking on ``_source_case`` from the start
    control 0.3 sin(6x) cos(5y) cos(400t), beta = 1e-3, control bounds -50..50, 4 iterations, max_armijo = 6, against the
    CPU loop: the bars of the drift-control test.  Coefficients (5e-4, 5e-6); measured on the CPU: trials [1, 2, 3, 2],
    smallest margin 5.2e-2."""
    N, Nt, dt, n, ls, wind, u0, uhat, c0 = source_inputs()
    uo, po, co, ho = cpu_source()
    assert ho["armijo_margin_min"] >= 1e-8 and max(ho["armijo_k"]) > 1
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind)
    try:
        u, p, c, h = solvers.pgd_source_control(prob, u0, uhat, c0, 1e-3, -50.0, 50.0, optim="alltime", increment="resolve",
                                                max_armijo=6, max_iters=4, tol=0.0,
                                                smoothness=solvers.Smoothness(*SOURCE_COEFFS))
    finally:
        prob.close()
    print(f"[smoothness] source PGD: device costs {h['cost']}, CPU {ho['cost']}; trials {h['armijo_k']}; state "
          f"{rel(u, uo):.2e}, control {rel(c, co):.2e}, adjoint {rel(p, po):.2e}")
    _compare_histories(h, ho)
    assert rel(u, uo) < ADJ_TOL and rel(c, co) < ADJ_TOL and rel(p, po) < ADJ_TOL


def _history_equal(h1, h0):
    return all(h1[key] == h0[key] for key in ("cost", "armijo_k", "armijo_margin", "used", "pairs", "step"))


def _check_active(h):
    assert len(h["cost"]) >= 1 and len(h["roughness_x"]) == len(h["roughness_t"]) == len(h["cost"])
    assert np.isfinite(h["cost"]).all() and np.isfinite(h["roughness_x"]).all() and np.isfinite(h["roughness_t"]).all()
    assert min(h["roughness_x"]) > 0 and min(h["roughness_t"]) > 0
    assert np.all(np.diff([h["cost0"]] + h["cost"]) <= 0)


def test_lbfgs_solidbody(hp, solvers, pgd_case):
    """lbfgs_solidbody: Smoothness(0, 0) gives the history of the run without the term bit for bit (a context each) and
    records the roughness; an active run has finite roughness histories and an accepted J + R that never increases; with
    control intervals the iterates of an active run stay piecewise constant bit for bit."""
    k = pgd_case
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    od = _Order(k["mesh"], True)
    c0 = od.to_dev(rough_start(k))

    def run(c_start, **kw):
        prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
        try:
            return solvers.lbfgs_solidbody(prob, od.to_dev(k["u0"]), od.to_dev(k["tgt"][Nt * n:]), c_start, k["beta"], 0.0,
                                           5.0, 3, max_armijo=6, **kw)
        finally:
            prob.close()

    (u0_, _, c0_, h0), (u1, _, c1, h1) = run(c0), run(c0, smoothness=solvers.Smoothness(0, 0))
    assert np.array_equal(bits(u1), bits(u0_)) and np.array_equal(bits(c1), bits(c0_))
    assert _history_equal(h1, h0) and h1["cost0"] == h0["cost0"]
    assert "roughness_x" not in h0 and len(h1["roughness_x"]) == len(h1["cost"]) and min(h1["roughness_t"]) > 0
    *_, h = run(c0, smoothness=solvers.Smoothness(2e-4, 4e-7))
    _check_active(h)
    ct = solvers.ControlIntervals.every(Nt, 4)
    cpc = ct.expand(ct.compact(c0, n))
    _, _, c, h = run(cpc, smoothness=solvers.Smoothness(2e-4, 4e-7), control_time=ct)
    _check_active(h)
    assert ct.contains(c, n) and not np.array_equal(c, cpc)


def test_lbfgs_source_control(hp, solvers):
    N, Nt, dt, n, ls, wind, u0, uhat, c0 = source_inputs()

    def run(c_start, **kw):
        prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind)
        try:
            return solvers.lbfgs_source_control(prob, u0, uhat, c_start, 1e-3, -50.0, 50.0, optim="alltime", max_armijo=6,
                                                max_iters=3, tol=0.0, **kw)
        finally:
            prob.close()

    (u0_, _, c0_, h0), (u1, _, c1, h1) = run(c0), run(c0, smoothness=solvers.Smoothness(0, 0))
    assert np.array_equal(bits(u1), bits(u0_)) and np.array_equal(bits(c1), bits(c0_))
    assert _history_equal(h1, h0) and h1["cost0"] == h0["cost0"]
    assert "roughness_x" not in h0 and len(h1["roughness_x"]) == len(h1["cost"])
    *_, h = run(c0, smoothness=solvers.Smoothness(*SOURCE_COEFFS))
    _check_active(h)
    ct = solvers.ControlIntervals.every(Nt, 4)
    cpc = ct.expand(ct.compact(c0, n))
    _, _, c, h = run(cpc, smoothness=solvers.Smoothness(*SOURCE_COEFFS), control_time=ct)
    _check_active(h)
    assert ct.contains(c, n) and not np.array_equal(c, cpc)


def test_pgd_with_control_intervals_stays_piecewise_constant(hp, solvers, pgd_case):
    """pgd_solidbody and pgd_source_control with ``control_time`` and an active term: every accepted control is constant
    on the intervals bit for bit, and the roughness in time of the last one is below the start's."""
    k = pgd_case
    n, Nt, dt = k["n"], k["Nt"], k["dt"]
    od = _Order(k["mesh"], True)
    ct = solvers.ControlIntervals.every(Nt, 3)
    cpc = ct.expand(ct.compact(od.to_dev(rough_start(k)), n))
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, k["N"] - 1), Nt, dt, om=OM, order=hp.ORDER_VERTEX)
    try:
        start = prob.ctx.smooth_cost(prob.ctx.array(cpc), Nt, dt)[0]
        _, _, c, h = solvers.pgd_solidbody(prob, od.to_dev(k["u0"]), od.to_dev(k["tgt"][Nt * n:]), cpc, k["beta"], 0.0, 5.0, 3,
                                           max_armijo=8, smoothness=solvers.Smoothness(2e-4, 4e-7), control_time=ct)
    finally:
        prob.close()
    assert ct.contains(c, n) and not np.array_equal(c, cpc)
    assert np.isfinite(h["roughness_t"]).all() and h["roughness_t"][-1] < start[1]
    N, Nt, dt, n, ls, wind, u0, uhat, c0 = source_inputs()
    ct = solvers.ControlIntervals.every(Nt, 3)
    cpc = ct.expand(ct.compact(c0, n))
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, wind)
    try:
        _, _, c, h = solvers.pgd_source_control(prob, u0, uhat, cpc, 1e-3, -50.0, 50.0, optim="alltime", increment="resolve",
                                                max_armijo=6, max_iters=3, tol=0.0, control_time=ct,
                                                smoothness=solvers.Smoothness(*SOURCE_COEFFS))
    finally:
        prob.close()
    assert ct.contains(c, n) and not np.array_equal(c, cpc) and np.isfinite(h["roughness_x"]).all()


# ------------------------------------------------------------------------------------------------ error paths, example
def test_error_paths(hp, solvers):
    N, Nt, dt = 5, 4, 1e-3
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, N - 1), Nt, dt, solvers.finaltime_exact_wind())
    ctx, n, tl = prob.ctx, prob.n, prob.tlen
    err = hp._lib.FemFctValueError
    try:
        c, u, p, out = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl)
        with pytest.raises(ValueError):
            solvers.Smoothness(-1)
        with pytest.raises(ValueError):
            solvers.Smoothness(0.0, np.nan)
        with pytest.raises(ValueError):                         # the fused linear-increment costs do not know the term
            solvers.pgd_source_control(prob, np.zeros(n), np.zeros(tl), np.zeros(tl), 1e-3, 0.0, 1.0, increment="linear",
                                       smoothness=solvers.Smoothness(1e-4, 0.0))
        with pytest.raises(ValueError):
            solvers.pgd_source_control(prob, np.zeros(n), np.zeros(tl), np.zeros(tl), 1e-3, 0.0, 1.0, increment="resolve",
                                       smoothness=(1e-4, 0.0))
        # the C entry points' argument checks
        for call, text in ((lambda: ctx.smooth_cost(None, Nt, dt), "null argument"),
                           (lambda: ctx.smooth_cost(c, 0, dt), "num_steps"),
                           (lambda: ctx.smooth_cost(c, Nt, dt, batch=0), "batch"),
                           (lambda: ctx.smooth_cost(c, Nt, 0.0), "dt"),
                           (lambda: ctx.smooth_rhs(None, 1.0, 1.0, Nt, dt, out), "null argument"),
                           (lambda: ctx.smooth_rhs(c, 1.0, 1.0, Nt, dt, None), "null argument"),
                           (lambda: ctx.smooth_rhs(c, 1.0, 1.0, 0, dt, out), "num_steps"),
                           (lambda: ctx.smooth_rhs(c, 1.0, 1.0, Nt, dt, out, batch=0), "batch"),
                           (lambda: ctx.smooth_rhs(c, 1.0, 1.0, Nt, -dt, out), "dt"),
                           (lambda: ctx.smooth_rhs(c, -1.0, 1.0, Nt, dt, out), "beta_x"),
                           (lambda: ctx.smooth_rhs(c, 1.0, np.nan, Nt, dt, out), "beta_t"),
                           (lambda: ctx.smooth_rhs(c, np.inf, 1.0, Nt, dt, out), "beta_x"),
                           (lambda: ctx.drift_gradient_rhs_smooth(None, u, p, 0.1, 1.0, 1.0, dt, out, Nt + 1), "null argument"),
                           (lambda: ctx.drift_gradient_rhs_smooth(c, u, p, 0.1, 1.0, 1.0, dt, None, Nt + 1), "null argument"),
                           (lambda: ctx.drift_gradient_rhs_smooth(c, u, p, 0.1, 1.0, 1.0, dt, out, 1), "num_steps"),
                           (lambda: ctx.drift_gradient_rhs_smooth(c, u, p, 0.1, 1.0, 1.0, 0.0, out, Nt + 1), "dt"),
                           (lambda: ctx.drift_gradient_rhs_smooth(c, u, p, 0.1, -1.0, 1.0, dt, out, Nt + 1), "beta_x"),
                           (lambda: ctx.drift_gradient_rhs_smooth(c, u, p, 0.1, 1.0, np.inf, dt, out, Nt + 1), "beta_t")):
            with pytest.raises(err, match=text):
                call()
        bare = importlib.import_module("fem-fct-pdeco_amd.device").Context(0)      # a context without the structured mesh
        try:
            with pytest.raises(err, match="structured mesh"):
                bare.smooth_cost(c, Nt, dt)
            with pytest.raises(err, match="structured mesh"):
                bare.smooth_rhs(c, 1.0, 1.0, Nt, dt, out)
            with pytest.raises(err, match="structured mesh"):
                bare.drift_gradient_rhs_smooth(c, u, p, 0.1, 1.0, 1.0, dt, out, Nt + 1)
        finally:
            bare.close()
        ctx.smooth_rhs(c, 1.0, 1.0, Nt, dt, out)                # still usable
        assert ctx.smooth_cost(c, Nt, dt)[0].tolist() == [0.0, 0.0]
    finally:
        prob.close()


def test_example_runs_at_a_reduced_size():
    """The example at its reduced size is the case of test_pgd_solidbody_smooths_the_control: after 4 iterations the run
    with the term ends with R_t = 26.9 against 104.1 and R_x = 0.211 against 0.289 (the CPU loop's values)."""
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "smooth_control_pdeco.py"), "--reduced"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    last = {}
    for ln in out.stdout.splitlines():
        for name in ("plain", "smooth"):
            for key in ("roughness_x", "roughness_t"):
                if ln.startswith(name) and f"{key}:" in ln:
                    last[name, key] = [float(v) for v in ln.split(f"{key}:")[1].split()]
    print(f"[smoothness] example: {last}")
    assert len(last) == 4 and all(len(v) == 4 and np.isfinite(v).all() for v in last.values())
    assert "two runs of 4 PGD iterations" in out.stdout
    assert last["smooth", "roughness_t"][-1] < 0.3 * last["plain", "roughness_t"][-1]
    assert last["smooth", "roughness_x"][-1] < 0.8 * last["plain", "roughness_x"][-1]
