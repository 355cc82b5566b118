"""Initial-state recovery on the device (solvers.initial_state_solidbody, solvers.OmegaLimitedMemory): the four primitives
femfct_initial_trials / femfct_initial_trial_stats / femfct_initial_gradient / femfct_omega_gram against NumPy and the
existing one-level entry points (bit for bit), and the loop against the CPU reference (initial_state_oracle.py) on case I,
which test_initial_state_oracle.py checks on the CPU."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import initial_state_oracle as io_

pytestmark = pytest.mark.gpu

ITERS = 5
LEVELS = 5                      # levels of the primitives' trajectories
MEMBERS = (1, 2, 10, 64)


def _mods():
    return importlib.import_module("fem-fct-pdeco_amd"), importlib.import_module("fem-fct-pdeco_amd.solvers")


def _rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(b)


def _ctx(nc):
    hp, _ = _mods()
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, 1)
    return hp, ctx


def _bytes(ctx, hp, count, values=None):
    """a device buffer of ``count`` bytes (uploaded from the uint8 array ``values`` when given)"""
    buf = ctx.empty((count + 7) // 8)
    if values is not None:
        v = np.zeros(8 * buf.count, dtype=np.uint8)
        v[:count] = values
        hp._lib.check(ctx.handle, hp._lib.lib.femfct_memcpy_h2d(ctx.handle, buf.ptr, v.ctypes.data, v.size))
    return buf


def _download_bytes(ctx, hp, buf, count):
    out = np.empty(count, dtype=np.uint8)
    hp._lib.check(ctx.handle, hp._lib.lib.femfct_memcpy_d2h(ctx.handle, out.ctypes.data, buf.ptr, count))
    return out


# --------------------------------------------------------------------------------------------------------------- trials
@pytest.mark.parametrize("nc", [12, 40])
def test_initial_trials_write_level_0_only_bitwise(nc):
    """169 nodes (one block of any row partition) and 1681 (several); K = 1, 2, 10, 64 members of 5 levels"""
    hp, ctx = _ctx(nc)
    n, Nt = ctx.n, LEVELS - 1
    tl = LEVELS * n
    lo, hi = -0.3, 0.9
    rng = np.random.default_rng(nc)
    try:
        v, d = rng.uniform(lo, hi, n), rng.standard_normal(n)
        vd, dd = ctx.array(v), ctx.array(d)
        for K in MEMBERS:
            steps = 2.0 * (1 / 2 ** np.arange(K))
            sentinel = rng.standard_normal(K * tl)
            uB = ctx.array(sentinel)
            ctx.initial_trials(vd, dd, steps, lo, hi, uB, Nt)
            got = uB.download().reshape(K, LEVELS, n)
            for k in range(K):
                assert got[k, 0].tobytes() == np.clip(v + steps[k] * d, lo, hi).tobytes(), (K, k)
            assert got[:, 1:].tobytes() == sentinel.reshape(K, LEVELS, n)[:, 1:].tobytes(), K
            assert np.any(got[0, 0] == lo) and np.any(got[0, 0] == hi) and np.any((got[0, 0] > lo) & (got[0, 0] < hi))
            ctx.initial_trials(vd, dd, steps, lo, hi, uB, Nt)
            assert uB.download().tobytes() == got.tobytes(), K
            # a step that clips everything: exactly the bounds
            big = np.where(np.arange(K) % 2 == 0, 1e300, -1e300)
            ctx.initial_trials(vd, dd, big, lo, hi, uB, Nt)
            got = uB.download().reshape(K, LEVELS, n)
            for k in range(K):
                assert np.array_equal(got[k, 0], np.where(big[k] * d > 0, hi, lo)), (K, k)
            uB.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- stats
@pytest.mark.parametrize("nc", [12, 40])
def test_initial_trial_stats_are_the_omega_norms_bitwise(nc):
    hp, ctx = _ctx(nc)
    n, Nt = ctx.n, LEVELS - 1
    tl = LEVELS * n
    rng = np.random.default_rng(10 + nc)
    try:
        v, vb = rng.standard_normal(n), rng.standard_normal(n)
        vd, vbd, zd = ctx.array(v), ctx.array(vb), ctx.zeros(n)
        for K in MEMBERS:
            mem = rng.standard_normal((K, LEVELS, n)) * 10.0 ** rng.integers(-2, 3, (K, 1, 1))
            mem[0, 0] = v                                   # a member equal to v, and (K >= 2) one equal to v_b
            if K >= 2:
                mem[1, 0] = vb
            uB = ctx.array(mem.ravel())
            st = ctx.initial_trial_stats(uB, vd, K, Nt, vb=vbd)
            assert st.shape == (K, 2)
            for k in range(K):
                at = uB.ptr + 8 * k * tl
                assert st[k, 0].tobytes() == ctx.l2_norm_sq_Omega(at, vbd)[0].tobytes(), (K, k)
                assert st[k, 1].tobytes() == ctx.l2_norm_sq_Omega(at, vd)[0].tobytes(), (K, k)
            assert st[0, 1] == 0.0 and st[0, 0] > 0
            if K >= 2:
                assert st[1, 0] == 0.0 and st[1, 1] > 0
            assert ctx.initial_trial_stats(uB, vd, K, Nt, vb=vbd).tobytes() == st.tobytes()
            # no background = a zero background = l2_norm_sq_Omega(., None)
            s0 = ctx.initial_trial_stats(uB, vd, K, Nt)
            assert s0.tobytes() == ctx.initial_trial_stats(uB, vd, K, Nt, vb=zd).tobytes()
            assert s0[K - 1, 0].tobytes() == ctx.l2_norm_sq_Omega(uB.ptr + 8 * (K - 1) * tl, None)[0].tobytes()
            # the levels past 0 and every other member may hold NaN
            k = K // 2
            bad = np.full((K, LEVELS, n), np.nan)
            bad[k, 0] = mem[k, 0]
            bd = ctx.array(bad.ravel())
            sn = ctx.initial_trial_stats(bd, vd, K, Nt, vb=vbd)
            assert sn[k].tobytes() == st[k].tobytes(), K
            assert K == 1 or np.isnan(np.delete(sn, k, axis=0)).all()
            uB.free(), bd.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("nc", [12, 40])
def test_initial_gradient_is_the_numpy_expression_bitwise(nc):
    hp, ctx = _ctx(nc)
    n = ctx.n
    lo, hi = 0.0, 0.8
    rng = np.random.default_rng(20 + nc)
    try:
        v = np.clip(rng.uniform(lo - 0.3, hi + 0.3, n), lo, hi)         # values at both bounds
        vb, p0 = rng.standard_normal(n), rng.standard_normal(n)
        p = np.full((LEVELS, n), np.nan)                                 # only level 0 may be read
        p[0] = p0
        vd, vbd, pd, g = ctx.array(v), ctx.array(vb), ctx.array(p.ravel()), ctx.empty(n)
        for beta0 in (1e-3, 0.37, 0.0):
            ctx.initial_gradient(pd, vd, beta0, g, vb=vbd)
            got = g.download()
            assert got.tobytes() == (beta0 * (v - vb) - p0).tobytes(), beta0
            ctx.initial_gradient(pd, vd, beta0, g)
            assert g.download().tobytes() == (beta0 * (v - np.zeros(n)) - p0).tobytes(), beta0
            if beta0 == 0.0:
                assert np.array_equal(got, -p0)
            # the fused free set is femfct_free_set's on the stored gradient, byte for byte
            mask, ref = _bytes(ctx, hp, n), _bytes(ctx, hp, n)
            ctx.initial_gradient(pd, vd, beta0, g, vb=vbd, v_lower=lo, v_upper=hi, mask=mask)
            assert g.download().tobytes() == got.tobytes()
            ctx.free_set(vd, g, lo, hi, n, ref)
            m = _download_bytes(ctx, hp, mask, n)
            assert np.array_equal(m, _download_bytes(ctx, hp, ref, n))
            assert np.array_equal(m, io_.free_set(v, got, lo, hi).astype(np.uint8)) and 0 < m.sum() < n
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("nc", [12, 40])
def test_omega_gram_matches_numpy(nc):
    """J = 1, 3, 7, 17; no mask, a random one, all bound.  |G_ij - ref| <= 1e-12 sqrt(G_ii G_jj), the bound
    test_gpu_lbfgs.py applies to femfct_q_gram for the reason stated there (the sums have at most 7 * 1681 terms per row
    tree here: four decades above f64 rounding, six below any indexing error)."""
    hp, ctx = _ctx(nc)
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    M = P1Assembler(SquareMesh(-1, 1, nc)).mass()
    n = ctx.n
    rng = np.random.default_rng(30 + nc)
    try:
        fields = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3) for _ in range(17)]
        dev = [ctx.array(f) for f in fields]
        masks = {"none": None, "random": rng.random(n) > 0.4, "bound": np.zeros(n, dtype=bool)}
        for name, mask in masks.items():
            md = None if mask is None else _bytes(ctx, hp, n, mask.astype(np.uint8))
            for J in (1, 3, 7, 17):
                G = ctx.omega_gram(dev[:J], mask=md)
                assert G.shape == (J, J) and G.tobytes() == G.T.copy().tobytes()
                assert ctx.omega_gram(dev[:J], mask=md).tobytes() == G.tobytes()
                if name == "bound":
                    assert np.array_equal(G, np.zeros((J, J)))
                    continue
                ref = io_.omega_gram(fields[:J], mask, M)
                bound = 1e-12 * np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
                print(f"nc={nc} {name} J={J}: max |G - ref| / bound = {np.max(np.abs(G - ref) / bound):.3e}")
                assert np.all(np.abs(G - ref) <= bound), (name, J)
                if mask is None:
                    for i in range(J):
                        assert G[i, i].tobytes() == ctx.l2_norm_sq_Omega(dev[i], None)[0].tobytes(), (J, i)
                else:
                    # a masked-out value is never read: NaN there changes nothing
                    nan = [ctx.array(np.where(mask, f, np.nan)) for f in fields[:J]]
                    assert ctx.omega_gram(nan, mask=md).tobytes() == G.tobytes(), J
                    for a in nan:
                        a.free()
            # one pointer twice
            G = ctx.omega_gram([dev[0], dev[1], dev[0]], mask=md)
            assert G[0, 0] == G[2, 2] == G[0, 2]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- loop against the oracle
@functools.lru_cache(maxsize=None)
def _case():
    return io_.case_i()


def _snap_obs():
    _, solvers = _mods()
    return solvers.Observations(_case()["Nt"], [5, 12, 20], weights=[0.5, 1.0, 2.0])


@functools.lru_cache(maxsize=None)
def _oracle_run(optim, memory, iters=ITERS, max_armijo=10):
    obs = _snap_obs() if optim == "snapshots" else None
    mode = "alltime" if optim == "snapshots" else optim
    u, p, v, h = io_.run(_case(), mode, memory, iters, obs=obs, max_armijo=max_armijo)
    for a in (u, p, v):
        a.setflags(write=False)
    return u, p, v, h


def _device_run(optim, memory, iters=ITERS, speculative=True, obs=None, max_armijo=10, s0=None, uhat=None, vertex=False):
    """``vertex``: the problem in the device's vertex order (the order of the one-workgroup step kernel), the data
    permuted on the way in and the results on the way out"""
    hp, solvers = _mods()
    cs = _case()
    n = cs["n"]
    batch = max_armijo if speculative else 1
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40, batch=batch,
                                  order=hp.ORDER_VERTEX if vertex else hp._lib.ORDER_FENICS)
    v2d = prob.mesh.vertex_to_dof
    to_dev = (lambda a: np.ascontiguousarray(a.reshape(-1, n)[:, v2d]).ravel()) if vertex else (lambda a: a)
    try:
        if max_armijo > 10:
            print("kernel_regime(%d) = %d, kernel_regime(1) = %d" % (max_armijo, prob.ctx.kernel_regime(max_armijo),
                                                                     prob.ctx.kernel_regime(1)))
        if optim == "snapshots" and obs is None:
            obs = _snap_obs()
        mode = "alltime" if optim == "snapshots" else optim
        u, p, v, h = solvers.initial_state_solidbody(
            prob, to_dev(cs["c"]), to_dev(io_.target(cs, mode) if uhat is None else uhat), to_dev(cs["v0"]), cs["beta0"],
            cs["lo"], cs["hi"], iters, background=to_dev(cs["vb"]), memory=memory, s0=io_.S0[mode] if s0 is None else s0,
            max_armijo=max_armijo, optim=optim, obs=obs, speculative=speculative)
    finally:
        prob.close()
    if vertex:
        back = []
        for a in (u, p, v):
            b = np.empty((a.size // n, n))
            b[:, v2d] = a.reshape(-1, n)
            back.append(b.ravel())
        u, p, v = back
    return u, p, v, h


def _assert_same_run(dev, ora):
    """the gate and the tolerances of test_gpu_ensemble._assert_same_run (their origin: test_gpu_lbfgs.py)"""
    (u, p, v, h), (uo, po, vo, ho) = dev, ora
    print("device", h["cost0"], h["cost"], h["armijo_k"], h["used"], h["armijo_margin_min"])
    print("oracle", ho["cost0"], ho["cost"], ho["armijo_k"], ho["used"], ho["armijo_margin_min"])
    assert h["armijo_k"] == ho["armijo_k"] and h["used"] == ho["used"]
    assert h["pairs"] == ho["pairs"] and h["sweeps"] == ho["sweeps"] and not h["stalled"] and not ho["stalled"]
    assert np.allclose(h["cost"], ho["cost"], rtol=1e-9, atol=0)
    assert abs(h["cost0"] - ho["cost0"]) <= 1e-9 * abs(ho["cost0"])
    assert ho["armijo_margin_min"] > 1e-7 and h["armijo_margin_min"] > 1e-7
    assert np.allclose(h["tracking"], ho["tracking"], rtol=1e-9, atol=0)
    assert np.allclose(h["background"], ho["background"], rtol=1e-9, atol=0)
    assert np.allclose(np.array(h["tracking"]) + np.array(h["background"]), h["cost"], rtol=1e-12, atol=0)
    assert abs(h["tracking0"] + h["background0"] - h["cost0"]) <= 1e-12 * h["cost0"]
    assert u.shape == uo.shape and p.shape == po.shape and v.shape == vo.shape
    assert _rel(v, vo) < 1e-8 and _rel(u, uo) < 1e-8 and _rel(p, po) < 1e-8


@pytest.mark.parametrize("optim,memory,armijo_k", [("finaltime", 0, [1, 2, 2, 1, 2]), ("finaltime", 3, [1, 2, 2, 2, 3]),
                                                   ("alltime", 0, [1, 1, 2, 1, 2]), ("alltime", 3, [1, 4, 4, 4, 5])])
def test_initial_state_loop_matches_oracle_on_case_i(optim, memory, armijo_k):
    dev, ora = _device_run(optim, memory), _oracle_run(optim, memory)
    _assert_same_run(dev, ora)
    (u, p, v, h), cs = dev, _case()
    assert h["armijo_k"] == armijo_k
    assert h["used"] == (["g"] * 5 if memory == 0 else ["g", "qn", "qn", "qn", "qn"])
    assert v.min() >= cs["lo"] and v.max() <= cs["hi"]
    assert np.any(v == cs["hi"]) and np.any(v == cs["lo"]) == np.any(ora[2] == cs["lo"])
    assert np.array_equal(u[:cs["n"]], v)
    costs = [h["cost0"]] + h["cost"]
    assert all(b < a for a, b in zip(costs, costs[1:]))


def test_speculative_equals_sequential():
    """the same decisions, iterates to 1e-11 (test_gpu_lbfgs.py's bound between its two searches)"""
    (us, ps, vs, hs), (uq, pq, vq, hq) = _device_run("finaltime", 3), _device_run("finaltime", 3, speculative=False)
    assert hs["armijo_k"] == hq["armijo_k"] and hs["used"] == hq["used"] and hs["sweeps"] == hq["sweeps"]
    assert hs["pairs"] == hq["pairs"] and max(hs["armijo_k"]) > 1
    assert np.allclose(hs["cost"], hq["cost"], rtol=1e-11, atol=0)
    assert _rel(vs, vq) < 1e-11 and _rel(us, uq) < 1e-11 and _rel(ps, pq) < 1e-11


def test_snapshots_match_oracle():
    """Observations(20, [5, 12, 20], weights = [0.5, 1, 2]), the trajectory as target, memory 3, s0 = 16"""
    dev, ora = _device_run("snapshots", 3), _oracle_run("snapshots", 3)
    _assert_same_run(dev, ora)
    assert "qn" in dev[3]["used"]


@pytest.mark.parametrize("optim", ["finaltime", "alltime"])
def test_observation_corners_reproduce_the_named_modes(optim):
    _, solvers = _mods()
    cs = _case()
    obs = solvers.Observations.finaltime(cs["Nt"]) if optim == "finaltime" else solvers.Observations.alltime(cs["Nt"], cs["dt"])
    u, p, v, h = _device_run("snapshots", 3, iters=3, obs=obs, s0=io_.S0[optim], uhat=cs["traj"])
    un, pn, vn, hn = _device_run(optim, 3, iters=3)
    assert h["armijo_k"] == hn["armijo_k"] and h["used"] == hn["used"] and h["pairs"] == hn["pairs"]
    assert h["sweeps"] == hn["sweeps"]
    assert np.allclose(h["cost"], hn["cost"], rtol=1e-9, atol=0) and _rel(v, vn) < 1e-8


def test_wide_search_of_64_trials_matches_oracle():
    """max_armijo = 64 on a problem of batch 64 in vertex order, two iterations: the 64 trials of a search are one sweep,
    one workgroup per trajectory (the regime is printed: a tuning knob may select another)"""
    dev = _device_run("finaltime", 3, iters=2, max_armijo=64, vertex=True)
    _assert_same_run(dev, _oracle_run("finaltime", 3, 2, 64))
    assert dev[3]["armijo_k"] == [1, 2]


def test_argument_errors_leave_the_context_usable():
    hp, solvers = _mods()
    cs = _case()
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40, batch=10)
    ctx, n, tl, Nt = prob.ctx, cs["n"], cs["tl"], cs["Nt"]
    uhT = io_.target(cs, "finaltime")
    run = lambda c=cs["c"], uhat=uhT, v0=cs["v0"], beta0=cs["beta0"], lo=cs["lo"], hi=cs["hi"], **kw: \
        solvers.initial_state_solidbody(prob, c, uhat, v0, beta0, lo, hi, 1, **{"s0": 4.0, **kw})
    try:
        for kw in (dict(c=cs["c"][:-1]), dict(v0=cs["v0"][:-1]), dict(background=np.zeros(n + 1)), dict(uhat=cs["traj"]),
                   dict(uhat=uhT, optim="alltime"), dict(beta0=-1e-3), dict(beta0=np.nan), dict(beta0=np.inf),
                   dict(lo=0.9, hi=0.8), dict(max_armijo=11), dict(max_armijo=0), dict(optim="snapshots", uhat=cs["traj"]),
                   dict(optim="snapshots", uhat=uhT, obs=_snap_obs()), dict(optim="sometimes"), dict(memory=9)):
            with pytest.raises(ValueError):
                run(**kw)
        # the primitives
        a, b = ctx.zeros(2 * tl), ctx.zeros(n)
        with pytest.raises(ValueError):
            ctx.initial_trials(b, b, [], 0.0, 1.0, a, Nt)
        with pytest.raises(ValueError):
            ctx.initial_trials(b, b, np.ones(257), 0.0, 1.0, a, Nt)
        with pytest.raises(ValueError):
            ctx.initial_trials(b, b, [1.0], 1.0, 0.0, a, Nt)
        with pytest.raises(ValueError):
            ctx.initial_trials(b, None, [1.0], 0.0, 1.0, a, Nt)
        with pytest.raises(ValueError):
            ctx.initial_trial_stats(a, b, 0, Nt)
        with pytest.raises(ValueError):
            ctx.initial_trial_stats(a, None, 2, Nt)
        with pytest.raises(ValueError):
            ctx.initial_gradient(a, b, -1.0, b)
        with pytest.raises(ValueError):
            ctx.initial_gradient(None, b, 1.0, b)
        for bad in ([], [b] * 18, [b, None]):
            with pytest.raises(ValueError):
                ctx.omega_gram(bad)
        # still usable: one iteration runs, and a sequential search may be longer than the batch
        h = run()[3]
        assert len(h["cost"]) == 1 and h["cost"][0] < h["cost0"]
        assert np.allclose(run(max_armijo=11, speculative=False)[3]["cost"], h["cost"], rtol=1e-11, atol=0)
    finally:
        prob.close()


def test_example_runs():
    """examples/initial_state_solidbody_pdeco.py, two iterations of a reduced run (100 steps), as a child process"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "initial_state_solidbody_pdeco.py"), "--iters", "2", "--steps",
                          "100"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "tracking" in out.stdout and "background" in out.stdout and "   2  " in out.stdout
