"""GPU tests (-m gpu) of the lockstep regularisation sweep: femfct_trial_controls and femfct_member_costs against the
entry points they batch (bit for bit), and solvers.pgd_solidbody_lockstep against the CPU oracle's loop and against
pgd_solidbody run alone per problem, in every kernel regime.

Common set-up (that of test_gpu_traj.py::test_pgd_solidbody_matches_oracle_loop_...): u0 = exp(-15((x+0.2)^2+(y-0.1)^2)),
om = pi/40, eps = 0, c0 = 1, bounds [0, 5], gam = 1e-4; all-time target = forward solve at c = 2, final-time target =
exp(-15((x+0.1)^2+(y-0.2)^2)); Nt = 6, dt = 1e-3 * 80/(N-1), s0 = 8."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from regime_helpers import regime_knobs_default

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, OM, LO, HI, GAM, S0 = 6, np.pi / 40, 0.0, 5.0, 1e-4, 8.0
BETAS4 = [0.1, 0.03, 0.01, 0.001]
BETAS8 = [10.0 ** (-k / 2) for k in range(2, 10)]


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


# ---------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def case(N):
    """Oracle objects and inputs of the common set-up at N x N nodes, in DoF (FEniCS) order; computed once per N."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    om = SquareMesh(-1, 1, N - 1)
    asm = P1Assembler(om)
    n, dt = om.nodes, 1e-3 * 80 / (N - 1)
    tl = (NT + 1) * n
    sb = otraj.SolidBody(asm, om=OM)
    u0 = np.exp(-15 * ((om.x + 0.2) ** 2 + (om.y - 0.1) ** 2))[om.dof_to_vertex]
    uhat_T = np.exp(-15 * ((om.x + 0.1) ** 2 + (om.y - 0.2) ** 2))[om.dof_to_vertex]
    uhat_all = np.zeros(tl)
    uhat_all[:n] = u0
    otraj.solidbody_forward(sb, 2.0 * np.ones(tl), uhat_all, n, NT, dt)
    for a in (u0, uhat_T, uhat_all):
        a.setflags(write=False)
    return dict(mesh=om, sb=sb, n=n, dt=dt, tl=tl, u0=u0, finaltime=uhat_T, alltime=uhat_all, M=asm.mass())


@functools.lru_cache(maxsize=None)
def oracle_run(N, optim, beta, K, iters):
    """oracle.traj.solidbody_pgd_loop for one beta (DoF order): (u, c, hist); computed once, shared, read-only."""
    from oracle import traj as otraj
    cs = case(N)
    u, _, c, h = otraj.solidbody_pgd_loop(cs["sb"], cs["u0"], cs[optim], np.ones(cs["tl"]), beta, LO, HI, iters, cs["n"],
                                          NT, cs["dt"], GAM, S0, K, optim)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c, h


def to_dev(cs, a, order):
    """DoF order -> the device's order (per level)"""
    if order == 1:
        return np.array(a, dtype=np.float64)
    return np.ascontiguousarray(np.asarray(a).reshape(-1, cs["n"])[:, cs["mesh"].vertex_to_dof]).ravel()


def to_dof(cs, a, order):
    if order == 1:
        return a
    back = np.empty((a.size // cs["n"], cs["n"]))
    back[:, cs["mesh"].vertex_to_dof] = a.reshape(-1, cs["n"])
    return back.ravel()


def new_prob(hp, solvers, N, order):
    cs = case(N)
    return solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, N - 1), NT, cs["dt"], om=OM, order=order)


def dev_inputs(cs, optim, order):
    return to_dev(cs, cs["u0"], order), to_dev(cs, cs[optim], order), np.ones(cs["tl"])


def check_against_oracle(cs, order, res, N, optim, beta, K, iters):
    """the bars of the single-beta test: armijo_k equal, costs rtol 1e-9, margins allclose(1e-6, 1e-9), c and u 1e-8"""
    u, _, c, h = res
    u_o, c_o, h_o = oracle_run(N, optim, beta, K, iters)
    assert h["armijo_k"] == h_o["armijo_k"]
    assert np.allclose(h["cost"], h_o["cost"], rtol=1e-9, atol=0)
    for ms_d, ms_o in zip(h["armijo_margin"], h_o["armijo_margin"]):
        assert np.allclose(ms_d, ms_o, rtol=1e-6, atol=1e-9)
    assert rel(to_dof(cs, c, order), c_o) < 1e-8 and rel(to_dof(cs, u, order), u_o) < 1e-8


def check_against_single(res, single):
    """a problem of the lockstep run against pgd_solidbody alone (another batch size, maybe another regime: not bits)"""
    (u, _, c, h), (u_s, _, c_s, h_s) = res, single
    assert h["armijo_k"] == h_s["armijo_k"]
    assert np.allclose(h["cost"], h_s["cost"], rtol=1e-9, atol=0)
    assert rel(c, c_s) < 1e-8 and rel(u, u_s) < 1e-8


def single_run(hp, solvers, N, order, optim, beta, K, iters, tol=None):
    cs = case(N)
    prob = new_prob(hp, solvers, N, order)
    try:
        u0, uhat, c0 = dev_inputs(cs, optim, order)
        return solvers.pgd_solidbody(prob, u0, uhat, c0, beta, LO, HI, iters, GAM, S0, K, True, tol, optim=optim)
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 1. trial_controls
@pytest.mark.parametrize("N", [5, 21])
def test_trial_controls_equal_project_control_calls(hp, N):
    P, K = 3, 4
    n = N * N
    count = 4 * n                       # N = 5: 100 values, no multiple of the block
    rng = np.random.default_rng(N)
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1)
        c_h = 5.0 * rng.random((P, count))
        d_h = 4.0 * rng.standard_normal((P, count))
        steps = np.array([[s0p * (1 / 2 ** t) for t in range(K)] for s0p in (8.0, 1.0, 0.3)])    # distinct per problem
        c, d = ctx.array(c_h), ctx.array(d_h)
        out, ref = ctx.zeros(P * K * count), ctx.zeros(P * K * count)
        ctx.trial_controls(c, d, steps, P, K, LO, HI, count, out)
        for p in range(P):
            for t in range(K):
                ctx.project_control(c.ptr + 8 * p * count, steps[p, t], d.ptr + 8 * p * count, LO, HI,
                                    ref.ptr + 8 * (p * K + t) * count, count)
        got, want = out.download(), ref.download()
        assert np.array_equal(got, want)
        assert np.any(want == LO) and np.any(want == HI) and np.any((want > LO) & (want < HI))    # clips at both bounds
        with pytest.raises(hp.FemFctValueError):
            ctx.trial_controls(c, d, np.ones(257), 257, 1, LO, HI, 1, out)
        with pytest.raises(hp.FemFctValueError):
            ctx.trial_controls(c, d, np.ones(257), 1, 257, LO, HI, 1, out)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 2. member_costs
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("N", [5, 21, 46])
def test_member_costs_equal_cost_functional_and_norm_per_member(hp, N, order):
    n, Nt, dt = N * N, NT, 1e-3
    tl = (Nt + 1) * n
    rng = np.random.default_rng(100 * N + order)
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1, order)
        for P, K in ((3, 4), (1, 1)):
            betas = [0.1, 0.03, 0.001][:P]
            u_h, c_h = rng.standard_normal((P * K, tl)), 5.0 * rng.random((P * K, tl))
            cref_h = 5.0 * rng.random((P, tl))
            u, c, cref = ctx.array(u_h), ctx.array(c_h), ctx.array(cref_h)
            for optim in ("alltime", "finaltime"):
                usz = tl if optim == "alltime" else n
                uh = ctx.array(rng.standard_normal((P, usz)))
                for per in (False, True):
                    J_ref, d_ref = np.empty(P * K), np.empty(P * K)
                    for m in range(P * K):
                        p = m // K
                        tgt = uh.ptr + 8 * (p * usz if per else 0)
                        J_ref[m] = ctx.cost_functional(u.ptr + 8 * m * tl, tgt, c.ptr + 8 * m * tl, Nt, dt, betas[p], optim)[0]
                        d_ref[m] = ctx.l2_norm_sq_Q(c.ptr + 8 * m * tl, cref.ptr + 8 * p * tl, Nt, dt)[0]
                    J, dist = ctx.member_costs(u, uh, c, betas, P, K, Nt, dt, optim, cref=cref, uhat_per_problem=per)
                    assert np.array_equal(J, J_ref), (P, K, optim, per)
                    assert np.array_equal(dist, d_ref), (P, K, optim, per)
                    J2, none = ctx.member_costs(u, uh, c, betas, P, K, Nt, dt, optim, uhat_per_problem=per)
                    assert none is None and np.array_equal(J2, J_ref)
                uh.free()
            for a in (u, c, cref):
                a.free()
    finally:
        ctx.close()


def test_member_costs_beyond_65535_level_member_pairs(hp):
    """N = 5, Nt = 700, 96 members (701 x 96 = 67296 pairs, 13 MB per array): the existing entry points refuse the shape,
    so the reference is the CPU oracle, to 1e-12 relative (sums of < 2e4 terms of one sign in double: ~1e-14)."""
    from oracle import fct as ofct
    N, Nt, P, K, dt = 5, 700, 12, 8, 1e-3
    cs = case(N)
    n, M = cs["n"], cs["M"]
    tl = (Nt + 1) * n
    rng = np.random.default_rng(5)
    betas = [10.0 ** (-k / 4) for k in range(P)]
    u_h, c_h = rng.standard_normal((P * K, tl)), 5.0 * rng.random((P * K, tl))
    cref_h = 5.0 * rng.random((P, tl))
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1, 1)          # FEniCS order = the oracle's
        u, c, cref = ctx.array(u_h), ctx.array(c_h), ctx.array(cref_h)
        with pytest.raises(hp.FemFctValueError):
            ctx.cost_functional(u, u, c, Nt, dt, 0.1, "alltime", batch=P * K)
        for optim in ("alltime", "finaltime"):
            usz = tl if optim == "alltime" else n
            uh_h = rng.standard_normal((P, usz))
            uh = ctx.array(uh_h)
            J, dist = ctx.member_costs(u, uh, c, betas, P, K, Nt, dt, optim, cref=cref, uhat_per_problem=True)
            J_ref = np.array([ofct.cost_functional(u_h[m], uh_h[m // K], c_h[m], Nt, dt, M, betas[m // K], optim)
                              for m in range(P * K)])
            d_ref = np.array([ofct.l2_norm_sq_Q(c_h[m] - cref_h[m // K], Nt, dt, M) for m in range(P * K)])
            assert np.max(np.abs(J - J_ref) / np.abs(J_ref)) < 1e-12
            assert np.max(np.abs(dist - d_ref) / np.abs(d_ref)) < 1e-12
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 3. against the CPU loop
@pytest.mark.parametrize("optim", ["alltime", "finaltime"])
def test_lockstep_matches_oracle_loop_per_beta(hp, solvers, optim):
    """N = 21, vertex order (one-workgroup step), four beta, K = 4, two iterations.  CPU oracle with exactly these inputs:
    all-time armijo_k [1,2], [1,1], [1,1], [1,1], smallest margin 3.4e-4; final-time [4,4], [4,1], [4,1], [4,1], 3.3e-4."""
    N, order, K, iters = 21, 0, 4, 2
    cs = case(N)
    oracles = [oracle_run(N, optim, b, K, iters) for b in BETAS4]
    assert all(abs(m) >= 1e-7 for _, _, h in oracles for ms in h["armijo_margin"] for m in ms)
    assert len({tuple(h["armijo_k"]) for _, _, h in oracles}) >= 2
    prob = new_prob(hp, solvers, N, order)
    try:
        u0, uhat, c0 = dev_inputs(cs, optim, order)
        res = solvers.pgd_solidbody_lockstep(prob, u0, uhat, c0, BETAS4, LO, HI, iters, GAM, S0, K, optim=optim)
        assert len(res) == 4 and res.record["problems"] == [4, 4] and res.record["trials"] == [16, 16]
        for b, r in zip(BETAS4, res):
            check_against_oracle(cs, order, r, N, optim, b, K, iters)
            assert set(r[3]) >= {"cost", "armijo_k", "step", "rel_change", "armijo_margin", "armijo_margin_min", "wall"}
            assert r[3]["armijo_margin_min"] > 1e-7
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 4. every kernel regime
@pytest.mark.parametrize("N,order,betas,K,regime", [
    (21, 1, BETAS4, 4, ("REGIME_ROWS", "REGIME_STRIPS")),
    (46, 0, BETAS4, 4, ("REGIME_TILE32",)),
    (81, 0, BETAS4, 4, ("REGIME_PATCH64",)),
    (81, 0, BETAS8, 8, ("REGIME_MESH",)),
], ids=["rows-strips", "tile32", "patch64", "mesh-large-batch"])
def test_lockstep_in_every_kernel_regime(hp, solvers, N, order, betas, K, regime):
    """All-time mode, two iterations.  CPU oracle: N = 46 armijo_k [1,2], [1,1], [1,1], [1,1], smallest margin 1.4e-4;
    N = 81 with the eight beta [1,2] then seven [1,1], smallest margin 5.7e-5."""
    optim, iters, P = "alltime", 2, len(betas)
    cs = case(N)
    prob = new_prob(hp, solvers, N, order)
    try:
        if regime_knobs_default():
            assert prob.ctx.kernel_regime(P * K) in [getattr(hp._lib, r) for r in regime]
        u0, uhat, c0 = dev_inputs(cs, optim, order)
        res = solvers.pgd_solidbody_lockstep(prob, u0, uhat, c0, betas, LO, HI, iters, GAM, S0, K, optim=optim)
        assert res.record["trials"] == [P * K] * iters
        assert res.record["regime_trials"] == [prob.ctx.kernel_regime(P * K)] * iters
    finally:
        prob.close()
    for b, r in zip(betas, res):
        check_against_single(r, single_run(hp, solvers, N, order, optim, b, K, iters))
    for j in (0, P // 2, P - 1):
        h_o = oracle_run(N, optim, betas[j], K, iters)[2]
        assert h_o["armijo_margin_min"] >= 1e-7
        check_against_oracle(cs, order, res[j], N, optim, betas[j], K, iters)


# ---------------------------------------------------------------------------------------------- 5. P = 1
@pytest.mark.parametrize("optim", ["alltime", "finaltime"])
def test_one_problem_is_pgd_solidbody_bit_for_bit(hp, solvers, optim):
    """Fresh contexts: the sweep controller's budgets depend on a context's history."""
    N, order, K, iters, beta = 21, 0, 4, 2, 0.03
    cs = case(N)
    u_s, p_s, c_s, h_s = single_run(hp, solvers, N, order, optim, beta, K, iters)
    prob = new_prob(hp, solvers, N, order)
    try:
        u0, uhat, c0 = dev_inputs(cs, optim, order)
        res = solvers.pgd_solidbody_lockstep(prob, u0, uhat, c0, [beta], LO, HI, iters, GAM, S0, K, optim=optim)
    finally:
        prob.close()
    assert len(res) == 1
    u, p, c, h = res[0]
    assert np.array_equal(u, u_s) and np.array_equal(p, p_s) and np.array_equal(c, c_s)
    for key in ("cost", "armijo_k", "step", "rel_change", "armijo_margin", "armijo_margin_min"):
        assert h[key] == h_s[key], key


# ---------------------------------------------------------------------------------------------- 6. stopping
def test_problems_stop_on_their_own_and_leave_the_batch(hp, solvers):
    N, order, K, iters, optim = 21, 0, 4, 5, "alltime"
    cs = case(N)
    free = [single_run(hp, solvers, N, order, optim, b, K, iters) for b in BETAS4]
    # a tol strictly between two rel_change values of the free runs: the problem holding the smaller one stops there
    vals = sorted({v for r in free for v in r[3]["rel_change"][:-1]})
    assert len(vals) >= 2
    tol = None
    for lo_v, hi_v in zip(vals[:-1], vals[1:]):
        t = 0.5 * (lo_v + hi_v)
        counts = [next((k + 1 for k, v in enumerate(r[3]["rel_change"]) if v < t), iters) for r in free]
        if min(counts) < iters and max(counts) == iters:
            tol = t
            break
    assert tol is not None, [r[3]["rel_change"] for r in free]
    singles = [single_run(hp, solvers, N, order, optim, b, K, iters, tol=tol) for b in BETAS4]
    counts = [len(s[3]["cost"]) for s in singles]
    assert min(counts) < iters and max(counts) == iters, counts
    prob = new_prob(hp, solvers, N, order)
    try:
        u0, uhat, c0 = dev_inputs(cs, optim, order)
        res = solvers.pgd_solidbody_lockstep(prob, u0, uhat, c0, BETAS4, LO, HI, iters, GAM, S0, K, tol=tol, optim=optim)
    finally:
        prob.close()
    for r, s in zip(res, singles):
        assert len(r[3]["cost"]) == len(s[3]["cost"])
        check_against_single(r, s)
    sizes = res.record["problems"]
    assert sizes == [sum(1 for n_it in counts if n_it > it) for it in range(len(sizes))]
    assert sizes[0] == 4 and sizes[-1] < 4 and all(a >= b for a, b in zip(sizes, sizes[1:]))
    assert res.record["trials"] == [K * s for s in sizes]


# ---------------------------------------------------------------------------------------------- 7. errors
def test_lockstep_argument_errors(hp, solvers):
    N, order, K = 21, 0, 4
    cs = case(N)
    prob = new_prob(hp, solvers, N, order)
    try:
        u0, uhat, c0 = dev_inputs(cs, "alltime", order)
        run = lambda **kw: solvers.pgd_solidbody_lockstep(**{**dict(
            prob=prob, u0=u0, uhat=uhat, c0=c0, betas=BETAS4, c_lower=LO, c_upper=HI, iters=1, gam=GAM, s0=S0,
            max_armijo=K, optim="alltime"), **kw})
        with pytest.raises(ValueError, match="snapshots"):
            run(optim="snapshots")
        with pytest.raises(ValueError):
            run(max_armijo=65)                          # 4 x 65 = 260 > 256
        with pytest.raises(ValueError):
            run(betas=[])
        with pytest.raises(ValueError):
            run(c0=np.ones(cs["tl"] - 1))
        with pytest.raises(ValueError):
            run(c0=np.ones((3, cs["tl"])))
        with pytest.raises(ValueError):
            run(uhat=uhat[:-1])
        with pytest.raises(ValueError):
            run(uhat=np.ones((3, cs["tl"])))
        bad = np.ones((4, cs["tl"]))
        bad[2, cs["tl"] // 2] = np.nan                  # NaN in one problem's start control: the sweep fails, as alone
        with pytest.raises(hp.NotConverged):
            run(c0=bad)
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 8. example
def test_lockstep_example_prints_eight_finite_costs():
    ex = os.path.join(ROOT, "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "c5_beta_lockstep.py"), "--steps", "6", "--iters", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("beta = ")]
    assert len(lines) == 8
    costs = [float(ln.split("=")[-1]) for ln in lines]
    assert all(np.isfinite(c) and c > 0 for c in costs)
