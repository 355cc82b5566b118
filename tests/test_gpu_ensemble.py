"""Ensemble drift control on the device (solvers.Ensemble, solvers.ensemble_solidbody): the two primitives
femfct_ensemble_drift_gradient_rhs / femfct_ensemble_costs against the single-scenario entry points (bit for bit) and
NumPy, and the loop against the CPU reference (ensemble_oracle.py) on case E, which test_ensemble_oracle.py checks on the
CPU."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ensemble_oracle as eo

pytestmark = pytest.mark.gpu

ITERS = 5


def _mods():
    return importlib.import_module("fem-fct-pdeco_amd"), importlib.import_module("fem-fct-pdeco_amd.solvers")


def _rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(b)


def _weights(rng, S):
    """random weights with a zero among them (S >= 2), normalised"""
    w = rng.random(S) + 0.1
    if S >= 2:
        w[S // 2] = 0.0
    return w / w.sum()


# ------------------------------------------------------------------------------------------------------- rhs primitive
@pytest.mark.parametrize("nc", [12, 40])
def test_ensemble_rhs_primitive(nc):
    """13 x 13 (one block of the row partition) and 41 x 41 nodes (several), 5 levels, S = 1, 2, 3, 7, 64.  Bitwise: S = 1
    and two equal scenarios with weights (1/2, 1/2) are drift_gradient_rhs, a NaN-filled scenario of weight 0 changes
    nothing, two calls agree.  Against NumPy, formed in the stated order from S single calls with beta = 0 plus the beta
    term: |out - ref| <= 1e-12 (|beta M c| + sum_s pi_s |G_s|) row by row (the sum has S + 1 terms: rounding is
    (S + 1) 1.1e-16 <= 8e-15 of that bound's right-hand side, an indexing error is O(1) of it)."""
    hp, _ = _mods()
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, 1)
    n, levels, beta = ctx.n, 5, 0.37
    tl = levels * n
    rng = np.random.default_rng(nc)
    try:
        c = rng.standard_normal(tl)
        cd, out, one = ctx.array(c), ctx.empty(tl), ctx.empty(tl)
        zero = ctx.zeros(tl)
        for S in (1, 2, 3, 7, 64):
            u, p = rng.standard_normal((S, tl)), rng.standard_normal((S, tl))
            w = _weights(rng, S)
            ud, pd = ctx.array(u.ravel()), ctx.array(p.ravel())
            ctx.ensemble_drift_gradient_rhs(cd, ud, pd, w, beta, out, levels)
            got = out.download()
            ctx.ensemble_drift_gradient_rhs(cd, ud, pd, w, beta, out, levels)
            assert out.download().tobytes() == got.tobytes(), S
            # the single calls: G_s = -(rhs with beta = 0), beta M c = -(rhs with p = 0)
            ctx.drift_gradient_rhs(cd, zero, zero, beta, one, levels)
            bmc = -one.download()
            G = []
            for s in range(S):
                ctx.drift_gradient_rhs(cd, ud.ptr + 8 * s * tl, pd.ptr + 8 * s * tl, 0.0, one, levels)
                G.append(-one.download())
            acc, mag = None, np.abs(bmc)
            for s in range(S):
                if w[s] == 0:
                    continue
                acc = w[s] * G[s] if acc is None else acc + w[s] * G[s]
                mag = mag + w[s] * np.abs(G[s])
            ref = -(bmc + acc)
            excess = np.abs(got - ref) / (1e-12 * mag)
            print(f"nc={nc} S={S}: max |out - ref| / bound = {excess.max():.3e}")
            assert np.all(np.abs(got - ref) <= 1e-12 * mag), (S, excess.max())
            # a zero-weight scenario full of NaN is never read
            if S >= 2:
                k = S // 2
                un, pn = u.copy(), p.copy()
                un[k], pn[k] = np.nan, np.nan
                und, pnd = ctx.array(un.ravel()), ctx.array(pn.ravel())
                ctx.ensemble_drift_gradient_rhs(cd, und, pnd, w, beta, out, levels)
                assert out.download().tobytes() == got.tobytes(), S
                und.free(), pnd.free()
            # S = 1 and duplicated scenarios
            ctx.drift_gradient_rhs(cd, ud, pd, beta, one, levels)
            single = one.download()
            ctx.ensemble_drift_gradient_rhs(cd, ud, pd, [1.0], beta, out, levels)
            assert out.download().tobytes() == single.tobytes(), S
            dd, dp = ctx.array(np.concatenate([u[0], u[0]])), ctx.array(np.concatenate([p[0], p[0]]))
            ctx.ensemble_drift_gradient_rhs(cd, dd, dp, [0.5, 0.5], beta, out, levels)
            assert out.download().tobytes() == single.tobytes(), S
            for a in (ud, pd, dd, dp):
                a.free()
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------- costs primitive
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("nc", [12, 40])
def test_ensemble_costs_primitive(nc, windowed):
    """T[s] = obs_cost of member s, the norm and distance parts = l2_norm_sq_Q, J = the stated expression in NumPy: all
    bit for bit; 5 and 21 levels; S = 1 and S = 64 give the same T[0]"""
    hp, _ = _mods()
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, 1)
    n, dt = ctx.n, 0.01
    rng = np.random.default_rng(7 * nc + windowed)
    try:
        win = ctx.array(rng.random(n)) if windowed else None
        for levels in (5, 21):
            Nt, tl = levels - 1, levels * n
            cw = rng.random(levels)
            cw[1] = 0.0
            cwd = ctx.array(cw)
            c, cref = rng.standard_normal(tl), rng.standard_normal(tl)
            cd, crd = ctx.array(c), ctx.array(cref)
            norm = ctx.l2_norm_sq_Q(cd, None, Nt, dt)[0]
            dist = ctx.l2_norm_sq_Q(cd, crd, Nt, dt)[0]
            T0 = None
            for S in (1, 2, 3, 7, 64):
                u, uh = rng.standard_normal((S, tl)), rng.standard_normal((S, tl))
                if T0 is not None:
                    u[0], uh[0] = first
                first = (u[0].copy(), uh[0].copy())
                ud, hd = ctx.array(u.ravel()), ctx.array(uh.ravel())
                w = _weights(rng, S)
                for beta in (2.0, 1e-3):
                    T, J, d = ctx.ensemble_costs(ud, hd, cwd, cd, w, beta, Nt, dt, window=win, cref=crd)
                    ref = ctx.obs_cost(ud, hd, cwd, Nt, window=win, batch=S)
                    assert T.tobytes() == ref.tobytes(), (levels, S)
                    assert np.float64(d).tobytes() == dist.tobytes()
                    track = None
                    for s in range(S):
                        if w[s] != 0:
                            track = w[s] * T[s] if track is None else track + w[s] * T[s]
                    assert np.float64(J).tobytes() == np.float64(track + (0.5 * beta) * norm).tobytes(), (levels, S, beta)
                    T2, J2, d2 = ctx.ensemble_costs(ud, hd, cwd, cd, w, beta, Nt, dt, window=win)
                    assert d2 is None and J2 == J and T2.tobytes() == T.tobytes()
                # a tracking sum that is exactly 0 (the weight on a scenario that sits on its target): J = the norm, beta = 2
                e = np.zeros(S)
                e[S - 1] = 1.0
                same = u.copy()
                same[S - 1] = uh[S - 1]
                sd = ctx.array(same.ravel())
                T, J, d = ctx.ensemble_costs(sd, hd, cwd, cd, e, 2.0, Nt, dt, window=win, cref=crd)
                assert T[S - 1] == 0.0 and np.float64(J).tobytes() == norm.tobytes()
                if T0 is None:          # S = 1: scenario 0 alone; the wider ensembles carry the same scenario 0
                    T0 = ctx.obs_cost(ud, hd, cwd, Nt, window=win, batch=1)[0]
                else:
                    assert ctx.ensemble_costs(ud, hd, cwd, cd, w, 0.0, Nt, dt, window=win)[0][0].tobytes() == T0.tobytes()
                for a in (ud, hd, sd):
                    a.free()
            for a in (cwd, cd, crd):
                a.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- loop against the oracle
@functools.lru_cache(maxsize=None)
def _case(optim, cycle=None):
    return eo.case_e(optim=optim, cycle=cycle)


@functools.lru_cache(maxsize=None)
def _oracle_run(optim, memory, starts=None, cycle=None, iters=ITERS):
    u, p, c, h = eo.run(_case(optim, cycle), iters, memory, starts=starts)
    for a in (u, p, c):
        a.setflags(write=False)
    return u, p, c, h


def _device_run(optim, memory, starts=None, cycle=None, iters=ITERS):
    hp, solvers = _mods()
    cs = _case(optim, cycle)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    ct = None if starts is None else solvers.ControlIntervals(cs["Nt"], list(starts))
    try:
        ens = solvers.Ensemble(cs["u0"], cs["uhat"], cs["weights"])
        if cycle is not None:
            print("kernel_regime(%d) = %d, kernel_regime(3) = %d" % (cycle, prob.ctx.kernel_regime(cycle),
                                                                     prob.ctx.kernel_regime(3)))
        return solvers.ensemble_solidbody(prob, ens, cs["c0"], cs["beta"], cs["lo"], cs["hi"], iters, memory=memory, s0=64.0,
                                          optim=cs["optim"], control_time=ct)
    finally:
        prob.close()


def _assert_same_run(dev, ora):
    """the tolerances and the gate of test_gpu_lbfgs.py (whose docstring gives their origin)"""
    (u, p, c, h), (uo, po, co, ho) = dev, ora
    print("device", h["cost0"], h["cost"], h["armijo_k"], h["used"], h["armijo_margin_min"])
    print("oracle", ho["cost0"], ho["cost"], ho["armijo_k"], ho["used"], ho["armijo_margin_min"])
    assert h["armijo_k"] == ho["armijo_k"] and h["used"] == ho["used"]
    assert h["pairs"] == ho["pairs"] and h["sweeps"] == ho["sweeps"] and not h["stalled"] and not ho["stalled"]
    assert np.allclose(h["cost"], ho["cost"], rtol=1e-9, atol=0)
    assert abs(h["cost0"] - ho["cost0"]) <= 1e-9 * abs(ho["cost0"])
    assert ho["armijo_margin_min"] > 1e-7 and h["armijo_margin_min"] > 1e-7
    assert np.allclose(np.array(h["scenario_costs"]), np.array(ho["scenario_costs"]), rtol=1e-9, atol=0)
    assert np.allclose(h["worst"], ho["worst"], rtol=1e-9, atol=0)
    assert np.allclose(h["control_cost"], ho["control_cost"], rtol=1e-6, atol=0)     # (a difference of two costs)
    assert u.shape == uo.shape and p.shape == po.shape
    assert _rel(c, co) < 1e-8 and _rel(u, uo) < 1e-8 and _rel(p, po) < 1e-8


@pytest.mark.parametrize("optim,memory,armijo_k", [("finaltime", 0, [4, 2, 4, 3, 4]), ("finaltime", 3, [4, 4, 6, 6, 6]),
                                                   ("alltime", 3, [1, 5, 6, 7, 6])])
def test_ensemble_loop_matches_oracle_on_case_e(optim, memory, armijo_k):
    dev, ora = _device_run(optim, memory), _oracle_run(optim, memory)
    _assert_same_run(dev, ora)
    h, cs = dev[3], _case(optim)
    assert h["armijo_k"] == armijo_k
    assert h["used"] == (["g"] * 5 if memory == 0 else ["g", "qn", "qn", "qn", "qn"])
    assert dev[2].min() >= cs["lo"] and dev[2].max() <= cs["hi"]
    if (optim, memory) == ("finaltime", 0):
        assert np.any(dev[2] == cs["lo"]) and np.any(dev[2] == cs["hi"])


def test_single_scenario_is_lbfgs_solidbody():
    """S = 1 against lbfgs_solidbody, sequential search, the same Observations: the same decisions, iterates to 1e-11
    (test_gpu_lbfgs.py's bound between its speculative and its sequential run)"""
    hp, solvers = _mods()
    cs = _case("alltime")
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    obs = solvers.Observations(cs["Nt"], [5, 12, 20], weights=[0.5, 1.0, 2.0])
    try:
        kw = dict(memory=3, s0=64.0, optim="snapshots", obs=obs)
        u1, p1, c1, h1 = solvers.lbfgs_solidbody(prob, cs["u0"][0], cs["uhat"][0], cs["c0"], cs["beta"], cs["lo"], cs["hi"],
                                                 ITERS, speculative=False, **kw)
        ens = solvers.Ensemble(cs["u0"][:1], cs["uhat"][:1])
        u, p, c, h = solvers.ensemble_solidbody(prob, ens, cs["c0"], cs["beta"], cs["lo"], cs["hi"], ITERS, **kw)
    finally:
        prob.close()
    print(h["armijo_k"], h["used"], h["cost"])
    assert h["armijo_k"] == h1["armijo_k"] and h["used"] == h1["used"] and h["sweeps"] == h1["sweeps"]
    assert max(h["armijo_k"]) > 1
    assert np.allclose(h["cost"], h1["cost"], rtol=1e-11, atol=0)
    assert _rel(c, c1) < 1e-11 and _rel(u[0], u1) < 1e-11 and _rel(p[0], p1) < 1e-11


def test_piecewise_constant_controls_stay_piecewise_constant_bitwise():
    _, solvers = _mods()
    cs = _case("finaltime")
    ct = solvers.ControlIntervals.every(cs["Nt"], 5)
    starts = tuple(int(s) for s in ct.starts)
    dev = _device_run("finaltime", 3, starts)
    assert ct.contains(dev[2], cs["n"]) and not np.array_equal(dev[2], cs["c0"])
    _assert_same_run(dev, _oracle_run("finaltime", 3, starts))


def test_wide_ensemble_matches_oracle():
    """S = 64: case E's three scenarios cycled, uniform weights, two iterations"""
    dev, ora = _device_run("finaltime", 3, cycle=64, iters=2), _oracle_run("finaltime", 3, cycle=64, iters=2)
    assert dev[0].shape == (64, _case("finaltime")["tl"])
    _assert_same_run(dev, ora)


def test_argument_errors_leave_the_context_usable():
    hp, solvers = _mods()
    cs = _case("finaltime")
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    ctx, n, tl = prob.ctx, cs["n"], cs["tl"]
    args = (cs["c0"], cs["beta"], cs["lo"], cs["hi"], 1)
    try:
        for bad in ([-1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [np.nan, 1.0, 1.0], [1.0, 1.0]):
            with pytest.raises(ValueError):
                solvers.Ensemble(cs["u0"], cs["uhat"], bad)
        with pytest.raises(ValueError):
            solvers.Ensemble(cs["u0"][0], cs["uhat"])
        with pytest.raises(ValueError):
            solvers.Ensemble(cs["u0"], cs["uhat"][:2])
        ens = solvers.Ensemble(cs["u0"], cs["uhat"], cs["weights"])
        assert ens.S == 3 and abs(ens.weights.sum() - 1) < 1e-15
        with pytest.raises(ValueError):
            solvers.ensemble_solidbody(prob, ens, *args, optim="alltime")                # final-time targets
        with pytest.raises(ValueError):
            solvers.ensemble_solidbody(prob, ens, cs["c0"][:-1], *args[1:])
        with pytest.raises(ValueError):
            solvers.ensemble_solidbody(prob, solvers.Ensemble(cs["u0"][:, :-1], cs["uhat"]), *args)
        wide = solvers.Ensemble(np.zeros((257, n)), np.zeros((257, n)))
        with pytest.raises(ValueError):
            solvers.ensemble_solidbody(prob, wide, *args)
        with pytest.raises(ValueError, match="state bounds are not carried"):
            solvers.ensemble_solidbody(prob, ens, *args, state_bounds=solvers.StateBounds(cs["Nt"], upper=1.0))
        # the primitives
        a, out = ctx.zeros(3 * tl), ctx.empty(tl)
        for w in ([], [-1.0, 2.0], [0.0, 0.0], [np.inf, 1.0], np.ones(257)):
            with pytest.raises(ValueError):
                ctx.ensemble_drift_gradient_rhs(a, a, a, w, 1.0, out, cs["Nt"] + 1)
            with pytest.raises(ValueError):
                ctx.ensemble_costs(a, a, a, a, w, 1.0, cs["Nt"], cs["dt"])
        with pytest.raises(ValueError):
            ctx.ensemble_drift_gradient_rhs(a, a, None, [1.0], 1.0, out, cs["Nt"] + 1)
        with pytest.raises(ValueError):
            ctx.ensemble_costs(a, a, None, a, [1.0], 1.0, cs["Nt"], cs["dt"])
        # still usable: one iteration runs
        h = solvers.ensemble_solidbody(prob, ens, *args, s0=64.0)[3]
        assert len(h["cost"]) == 1 and h["cost"][0] < h["cost0"]
    finally:
        prob.close()


def test_example_runs():
    """examples/ensemble_solidbody_pdeco.py, two iterations, as a child process"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "ensemble_solidbody_pdeco.py"), "--iters", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ensemble cost" in out.stdout and "scenario 0's own optimum" in out.stdout
