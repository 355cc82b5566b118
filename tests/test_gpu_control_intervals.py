"""GPU tests (-m gpu) of controls that are piecewise constant in time: femfct_time_restrict / femfct_time_prolong against
the NumPy reference (control_intervals_oracle.py), and ``control_time=`` in the four projected-gradient loops against the
CPU loops of the same file on the set-ups of control_intervals_cases.py (whose Armijo margins test_control_intervals_oracle.py
checks to be >= 1e-8).

Kernel bar, derived: the device and the reference both form the L-term sum of the same products w_l x_l and divide by
the same W_k; a sum of L terms carries at most (L - 1) 2^-53 sum |w_l x_l| <= (L - 1) 2^-53 W_k max_l |x_l| of error in
any order, the division one rounding more, so |dev - ref| <= 4 L 2^-53 max_l |x_l| per node and interval."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import control_intervals_cases as cc
import control_intervals_oracle as cio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


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


# ---------------------------------------------------------------------------------------------- 1. the kernels
def patterns(levels):
    """the four patterns that fit ``levels`` levels, and where an interval can be longer than a wave's run (8 levels)
    or a block's chunk (32), intervals of 20: one chunk, several waves"""
    out = {"stationary": (0, levels), "identity": tuple(range(levels + 1))}
    if levels > 2:
        out["0-1-end"] = (0, 1, levels)
    if levels > 4:
        out["0-3-4-end"] = (0, 3, 4, levels)
    if levels > 20:
        out["every-20"] = tuple(range(0, levels, 20)) + (levels,)
    return out


def bound(x, starts, levels, n):
    """4 L 2^-53 max_{l in k} |x_l| per interval and node: (B, K, n)"""
    a = np.abs(x.reshape(-1, levels, n))
    return np.stack([4 * (e - s) * U * a[:, s:e].max(axis=1) for s, e in zip(starts[:-1], starts[1:])], axis=1)


KERNEL_SHAPES = [(5, 2), (5, 7), (5, 251), (21, 2), (21, 7), (21, 41)]


@pytest.mark.parametrize("N,levels", KERNEL_SHAPES, ids=[f"n{N * N}-L{L}" for N, L in KERNEL_SHAPES])
def test_restrict_and_prolong_vs_numpy(hp, N, levels):
    """n = 25 and n = 441 (no multiple of 64: seven tiles, the last one partly filled); 2 levels (fewer than the waves of
    a block), 7 (every interval within one wave's run), 41 at n = 441 and 251 at n = 25 (several waves, and intervals
    longer than a block's chunk: the partials pass).  Batch 1 and 3 with distinct members; random data and data with
    magnitudes from 1e-8 to 1e8."""
    n, Nt = N * N, levels - 1
    tl = levels * n
    rng = np.random.default_rng(1000 * N + levels)
    wide = rng.standard_normal((3, tl)) * 10.0 ** rng.uniform(-8, 8, (3, tl))
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1)
        for name, starts in patterns(levels).items():
            K = len(starts) - 1
            for data in (rng.standard_normal((3, tl)), wide):
                x = ctx.array(data)
                out3, out1, back, twice = ctx.zeros(3 * K * n), ctx.zeros(K * n), ctx.zeros(3 * tl), ctx.zeros(3 * K * n)
                ctx.time_restrict(x, starts, Nt, out3, batch=3)
                got = out3.download().reshape(3, K, n)
                ref = np.stack([cio.restrict(data[b], starts, Nt, n) for b in range(3)])
                lim = bound(data, starts, levels, n)
                assert np.all(np.abs(got - ref) <= lim), (name, float(np.max(np.abs(got - ref) / np.maximum(lim, 1e-300))))
                for k, (s, e) in enumerate(zip(starts[:-1], starts[1:])):       # one level: that level, exactly
                    if e - s == 1:
                        assert np.array_equal(got[:, k], data.reshape(3, levels, n)[:, s]), (name, k)
                for b in range(3):                                                # a member alone: the same bits
                    ctx.time_restrict(x.ptr + 8 * b * tl, starts, Nt, out1, batch=1)
                    assert np.array_equal(out1.download().reshape(K, n), got[b]), (name, b)
                ctx.time_restrict(x, starts, Nt, twice, batch=3)                  # again: the same bits
                assert np.array_equal(twice.download().reshape(3, K, n), got), name
                ctx.time_prolong(out3, starts, Nt, back, batch=3)
                full = back.download().reshape(3, tl)
                assert np.array_equal(full, np.stack([cio.prolong(got[b], starts, Nt) for b in range(3)])), name
                # the projection in place, and applied twice: the mean of L equal values, to the same bound
                ctx.time_project(x, starts, Nt, twice, batch=3)
                once = x.download().reshape(3, tl)
                assert np.array_equal(once, full), name
                ctx.time_project(x, starts, Nt, twice, batch=3)
                again = x.download().reshape(3, tl)
                lim2 = np.stack([cio.prolong(bound(once, starts, levels, n)[b], starts, Nt) for b in range(3)])
                assert np.all(np.abs(again - once) <= lim2), name
                if name == "identity":
                    assert np.array_equal(once, data) and np.array_equal(again, data)
                for a in (x, out3, out1, back, twice):
                    a.free()
    finally:
        ctx.close()


def test_bad_starts_raise(hp):
    N, Nt = 5, 6
    n = N * N
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1)
        x, out = ctx.zeros((Nt + 1) * n), ctx.zeros((Nt + 1) * n)
        for bad in ((0, 3, 3, 7), (0, 4, 2, 7), (1, 7), (0, 6), (0, 8), (0, 3, 4, 5, 6, 7, 8), (0,)):
            with pytest.raises(ValueError):
                ctx.time_restrict(x, bad, Nt, out)
            with pytest.raises(ValueError):
                ctx.time_prolong(x, bad, Nt, out)
        with pytest.raises(ValueError):
            ctx.time_restrict(x, (0, 7), Nt, out, batch=0)
        with pytest.raises(ValueError):
            ctx.time_restrict(None, (0, 7), Nt, out)
        ctx.time_restrict(x, (0, 7), Nt, out)          # the context still works
        ctx.synchronize()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 2. solid body
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
    return solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, N - 1), cc.NT, cc.sb_case(N)["dt"], om=cc.OM, order=order)


def check_against_oracle(cs, order, res, ref):
    """test_gpu_lockstep.py's bars: armijo_k equal, costs rtol 1e-9, margins allclose(1e-6, 1e-9), c and u 1e-8"""
    u, _, c, h = res
    u_o, c_o, h_o = ref
    assert h["armijo_k"] == h_o["armijo_k"]
    assert np.allclose(h["cost"], h_o["cost"], rtol=1e-9, atol=0)
    for ms_d, ms_o in zip(h["armijo_margin"], h_o["armijo_margin"]):
        assert np.allclose(ms_d, ms_o, rtol=1e-6, atol=1e-9)
    assert rel(to_dof(cs, c, order), c_o) < 1e-8 and rel(to_dof(cs, u, order), u_o) < 1e-8


def check_against_single(res, single):
    (u, _, c, h), (u_s, _, c_s, h_s) = res, single
    assert h["armijo_k"] == h_s["armijo_k"]
    assert np.allclose(h["cost"], h_s["cost"], rtol=1e-9, atol=0)
    assert rel(c, c_s) < 1e-8 and rel(u, u_s) < 1e-8


def single_run(hp, solvers, N, order, optim, ct, beta=cc.BETA, K=cc.K_SB, iters=cc.ITERS_SB, speculative=True):
    cs = cc.sb_case(N)
    prob = new_prob(hp, solvers, N, order)
    try:
        return solvers.pgd_solidbody(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs[optim], order), np.ones(cs["tl"]),
                                     beta, cc.LO, cc.HI, iters, cc.GAM, cc.S0, K, speculative, None, optim=optim,
                                     control_time=ct)
    finally:
        prob.close()


@pytest.mark.parametrize("speculative", [True, False], ids=["speculative", "sequential"])
@pytest.mark.parametrize("order", [0, 1], ids=["vertex", "fenics"])
@pytest.mark.parametrize("N,optim,ivl", cc.SB_CASES)
def test_pgd_solidbody_vs_cpu_loop(hp, solvers, N, optim, ivl, order, speculative):
    cs = cc.sb_case(N)
    ct = solvers.ControlIntervals(cc.NT, cc.INTERVALS[ivl])
    ref = cc.sb_oracle(N, optim, ivl)
    assert ref[2]["armijo_margin_min"] >= cc.MARGIN_BAR
    res = single_run(hp, solvers, N, order, optim, ct, speculative=speculative)
    check_against_oracle(cs, order, res, ref)
    assert ct.contains(res[2], cs["n"])
    assert ct.compact(res[2], cs["n"]).shape == (ct.K, cs["n"])


def test_named_wrappers_pass_control_time_through(hp, solvers):
    N, order = 5, 1
    cs = cc.sb_case(N)
    ct = solvers.ControlIntervals.stationary(cc.NT)
    for optim, fn in (("alltime", solvers.pgd_solidbody_alltime), ("finaltime", solvers.pgd_solidbody_finaltime)):
        prob = new_prob(hp, solvers, N, order)
        try:
            res = fn(prob, cs["u0"], cs[optim], np.ones(cs["tl"]), cc.BETA, cc.LO, cc.HI, cc.ITERS_SB, cc.GAM, cc.S0, cc.K_SB,
                     control_time=ct)
        finally:
            prob.close()
        check_against_oracle(cs, order, res, cc.sb_oracle(N, optim, "stationary"))


def test_pgd_solidbody_snapshots_stationary(hp, solvers):
    N, order = 21, 0
    cs = cc.sb_case(N)
    obs, u_o, c_o, h_o = cc.snap_oracle(solvers.Observations)
    assert h_o["armijo_margin_min"] >= cc.MARGIN_BAR
    ct = solvers.ControlIntervals.stationary(cc.NT)
    obs_dev = solvers.Observations(cc.NT, obs.levels, window=to_dev(cs, obs.window, order))
    prob = new_prob(hp, solvers, N, order)
    try:
        res = solvers.pgd_solidbody_snapshots(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs["alltime"], order), obs_dev,
                                              np.ones(cs["tl"]), cc.BETA, cc.LO, cc.HI, cc.ITERS_SB, cc.GAM, cc.S0_SNAP,
                                              cc.K_SB, control_time=ct)
    finally:
        prob.close()
    check_against_oracle(cs, order, res, (u_o, c_o, h_o))
    assert ct.contains(res[2], cs["n"])


@pytest.mark.parametrize("N,optim,ivl", cc.LOCKSTEP_CASES)
def test_lockstep_vs_cpu_loop_and_single_runs(hp, solvers, N, optim, ivl):
    """four beta, K = 4, two iterations: every problem against the CPU loop and against pgd_solidbody(control_time=) run
    alone.  N = 46 in vertex order: the mass solves of the K * P interval fields run beside tile-regime sweeps."""
    order = 0
    cs = cc.sb_case(N)
    ct = solvers.ControlIntervals(cc.NT, cc.INTERVALS[ivl])
    prob = new_prob(hp, solvers, N, order)
    try:
        if N == 46:
            assert prob.ctx.kernel_regime(4 * cc.K_LS) == hp._lib.REGIME_TILE32 or not regime_default()
        res = solvers.pgd_solidbody_lockstep(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs[optim], order),
                                             np.ones(cs["tl"]), cc.BETAS4, cc.LO, cc.HI, cc.ITERS_LS, cc.GAM, cc.S0, cc.K_LS,
                                             optim=optim, control_time=ct)
    finally:
        prob.close()
    assert len(res) == 4 and res.record["problems"] == [4] * cc.ITERS_LS
    for b, r in zip(cc.BETAS4, res):
        ref = cc.sb_oracle(N, optim, ivl, b, cc.K_LS, cc.ITERS_LS)
        assert ref[2]["armijo_margin_min"] >= cc.MARGIN_BAR
        check_against_oracle(cs, order, r, ref)
        assert ct.contains(r[2], cs["n"])
        check_against_single(r, single_run(hp, solvers, N, order, optim, ct, b, cc.K_LS, cc.ITERS_LS))


def regime_default():
    from regime_helpers import regime_knobs_default
    return regime_knobs_default()


def test_identity_intervals_return_the_bits_of_the_free_loop(hp, solvers):
    """fresh contexts (the sweep controller's budgets depend on a context's history)"""
    N, order = 21, 0
    for optim in ("alltime", "finaltime"):
        u0, _, c0, h0 = single_run(hp, solvers, N, order, optim, None)
        u, _, c, h = single_run(hp, solvers, N, order, optim, solvers.ControlIntervals.identity(cc.NT))
        assert np.array_equal(u, u0) and np.array_equal(c, c0) and h["cost"] == h0["cost"]


# ---------------------------------------------------------------------------------------------- 3. source control
@pytest.mark.parametrize("increment", ["linear", "resolve"])
def test_pgd_source_control_stationary(hp, solvers, increment):
    """the reaction problem at 11 x 11 nodes / 10 steps, three iterations, at test_gpu_reaction_source.py's bars: the
    decisions of the CPU loop, costs to 1e-10, controls to 1e-9, state and adjoint to 1e-8, margins to 1e-8 absolute"""
    pr, (uo, po, co, ho) = cc.src_oracle(solvers.finaltime_exact_fields, solvers.finaltime_exact_wind(), increment)
    assert ho["armijo_margin_min"] >= cc.MARGIN_BAR
    n, Nt, dt, S = pr["n"], pr["Nt"], pr["dt"], cc.SRC
    tl = (Nt + 1) * n
    ct = solvers.ControlIntervals.stationary(Nt)
    prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, S["nc"]), Nt, dt, pr["wind"], pr["F"]["g"],
                                               eps=S["eps"], adjoint_mass=pr["sigma"])
    try:
        ug, pg, cg, hg = solvers.pgd_source_control(prob, pr["u0"], pr["uhat_T"], np.zeros(tl), S["beta"], S["lo"], S["hi"],
                                                    g=pr["F"]["f"], optim="finaltime", increment=increment,
                                                    max_iters=S["iters"], tol=0.0, stop="cost", control_time=ct)
    finally:
        prob.close()
    dm = max(abs(a - b) for mg, mo in zip(hg["armijo_margin"], ho["armijo_margin"]) for a, b in zip(mg, mo))
    dc = max(abs(a - b) / abs(b) for key in ("cost", "cost_state") for a, b in zip(hg[key], ho[key]))
    print(f"[control intervals] source control {increment}: armijo_k {hg['armijo_k']} (cpu {ho['armijo_k']}), cost {dc:.3e}, "
          f"control {rel(cg, co):.3e}, state {rel(ug, uo):.3e}, adjoint {rel(pg, po):.3e}, margins {dm:.3e}")
    assert hg["iterations"] == S["iters"] == len(ho["cost"])
    assert hg["armijo_k"] == ho["armijo_k"]
    assert dc <= 1e-10
    assert rel(cg, co) <= 1e-9
    assert rel(ug, uo) <= 1e-8 and rel(pg, po) <= 1e-8
    assert [len(m) for m in hg["armijo_margin"]] == [len(m) for m in ho["armijo_margin"]] and dm <= 1e-8
    assert ct.contains(cg, n)


# ---------------------------------------------------------------------------------------------- 4. the PDE systems
@pytest.mark.parametrize("name", list(cc.SYSTEMS))
def test_system_pdeco_vs_restated_loop(hp, solvers, name):
    """13 x 13 nodes, 8 steps, at test_gpu_pdeco.py's bars: iterations and trial counts equal, costs rtol 1e-9, fields 1e-7"""
    problem, dt, per_step, growth, starts, iters, opts = cc.SYSTEMS[name]
    asm, ic, targets, ref = cc.sys_case(name)
    assert ref["armijo_margin_min"] >= cc.MARGIN_BAR
    ct = solvers.ControlIntervals(cc.SYS_NT, starts)
    V = hp.SquareMeshP1(0.0, 1.0, cc.SYS_NC)
    got = hp.projected_gradient_descent(problem, V, ic, targets, cc.SYS_NT, dt, control_per_step=per_step, growth=growth,
                                        control_time=ct, max_iter_GD=iters, tol=0.0, **opts)
    assert got["it"] == ref["it"] and not got["restored"]
    assert got["armijo_its"] == ref["armijo_its"]
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9)
    for key in ("c", "u", "p") + (("v", "q") if problem != "nonlinear" else ()):
        assert rel(got[key], ref[key]) < 1e-7, key
    assert ct.contains(got["c"], V.nodes)


# ---------------------------------------------------------------------------------------------- 5. errors
def test_error_paths(hp, solvers):
    CI = solvers.ControlIntervals
    V = hp.SquareMeshP1(0.0, 1.0, cc.SYS_NC)
    with pytest.raises(ValueError, match="control_per_step"):
        hp.SystemPDECO("schnak", V, cc.SYS_NT, 1e-3, control_time=CI(cc.SYS_NT, (0, 5, cc.SYS_NT + 1)))
    with pytest.raises(ValueError):
        hp.SystemPDECO("schnak", V, cc.SYS_NT, 1e-3, control_time=CI.stationary(cc.SYS_NT + 1))
    with hp.SystemPDECO("schnak", V, cc.SYS_NT, 1e-3, control_time=CI.stationary(cc.SYS_NT)):
        pass                                        # K = 1 fits the frozen sweep
    with hp.SystemPDECO("schnak", V, cc.SYS_NT, 1e-3, control_per_step=True, control_time=CI.every(cc.SYS_NT, 3)):
        pass
    N, order = 5, 1
    cs = cc.sb_case(N)
    ct = CI(cc.NT, cc.INTERVALS["0-3-4-7"])
    c_bad = np.ones(cs["tl"])
    c_bad[cs["n"] + 3] = 1.5                        # level 1 differs from level 0 inside interval 0
    c_ok = ct.expand(np.arange(1.0, 4.0)[:, None] * np.ones(cs["n"]))
    prob = new_prob(hp, solvers, N, order)
    try:
        args = (cs["u0"], cs["alltime"])
        tail = (cc.BETA, cc.LO, cc.HI, 1, cc.GAM, cc.S0, 2)
        with pytest.raises(ValueError, match="not constant"):
            solvers.pgd_solidbody(prob, *args, c_bad, *tail, optim="alltime", control_time=ct)
        with pytest.raises(ValueError, match="not constant"):
            solvers.pgd_solidbody_lockstep(prob, *args, np.stack([c_ok, c_bad]), [0.1, 0.01], cc.LO, cc.HI, 1, cc.GAM, cc.S0,
                                           2, optim="alltime", control_time=ct)
        with pytest.raises(ValueError):
            solvers.pgd_solidbody(prob, *args, c_ok, *tail, optim="alltime", control_time=CI.stationary(cc.NT + 1))
        u, _, c, _ = solvers.pgd_solidbody(prob, *args, c_ok, *tail, optim="alltime", control_time=ct)
        assert ct.contains(c, cs["n"]) and np.ptp(ct.compact(c, cs["n"]), axis=0).max() > 0     # three distinct fields
    finally:
        prob.close()
    pr, _ = cc.src_oracle(solvers.finaltime_exact_fields, solvers.finaltime_exact_wind(), "linear")
    prob = solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, cc.SRC["nc"]), pr["Nt"], pr["dt"], pr["wind"],
                                               pr["F"]["g"], eps=cc.SRC["eps"])
    try:
        with pytest.raises(ValueError, match="not constant"):
            solvers.pgd_source_control(prob, pr["u0"], pr["uhat_T"], pr["F"]["c"], 0.1, 0.0, 1.0, optim="finaltime",
                                       max_iters=1, control_time=CI.stationary(pr["Nt"]))
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 6. the example
def test_example_reduced_run_lowers_the_cost():
    ex = os.path.join(ROOT, "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "stationary_control_pdeco.py"), "--reduced", "--iters", "3"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    costs = [float(ln.split("J =")[1].split()[0]) for ln in out.stdout.splitlines() if "J =" in ln]
    assert len(costs) == 4 and costs[-1] < costs[0]
    assert "constant in time: True" in out.stdout
