"""L1-sparse controls on the device (solvers.prox_solidbody, solvers.prox_source_control): the three primitives
femfct_prox_trials / femfct_l1_norm_Q / femfct_sparse_trial_stats against NumPy and against the primitives they fuse, and
the loops against the CPU reference loop (prox_oracle.py) on the cases test_prox_oracle.py checks on the CPU."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lbfgs_oracle as lo
import prox_oracle as po

pytestmark = pytest.mark.gpu

BOXES = [(-0.1, 0.5), (0.2, 1.0), (-1.0, -0.2)]
ALPHAS = (0.0, 1e-3, 0.7)
COUNTS = [n * levels for n in (36, 169, 1681) for levels in (1, 2, 8)] + [1681 * 3]


def _mods():
    return importlib.import_module("fem-fct-pdeco_amd"), importlib.import_module("fem-fct-pdeco_amd.solvers")


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def _mesh(nc):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    omesh = SquareMesh(-1, 1, nc)
    M = P1Assembler(omesh).mass()
    return omesh.nodes, omesh.vertex_to_dof, M, po.lumped_mass(M)


def _to_dev(x, n, v2d, order):
    return x if order == 1 else np.ascontiguousarray(x.reshape(-1, n)[:, v2d]).reshape(-1)


def _planted(rng, count, alpha, lo_, hi_):
    """c and d with, for every trial t, values whose x = c + s_t d is exactly +-tau_t (c = 0, d = +-alpha), values far outside
    the box on both sides, x = 0 and -0.0, and values that land exactly on a bound after the threshold (alpha = 0)"""
    c = rng.uniform(lo_ - 0.3, hi_ + 0.3, count)
    d = rng.standard_normal(count)
    m = min(count, 12)
    c[:m] = ([0.0, 0.0, 0.0, -0.0, lo_, hi_, 0.0, 0.0, lo_, hi_, 0.25, -0.25])[:m]
    d[:m] = ([alpha, -alpha, 0.0, -0.0, 0.0, 0.0, 1e9, -1e9, -1.0, 1.0, -alpha, alpha])[:m]
    return c, d


# ---------------------------------------------------------------------------------------------------- prox_trials
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("box", BOXES)
def test_prox_trials_equal_the_numpy_expression(box, order):
    """every count (n = 36, 169, 1681 with 1, 2, 8 levels, and 1681 * 3: odd, the scalar kernel), K = 1, 2, 10, 16,
    alpha = 0, 1e-3, 0.7, with g and sources, sources without g, and neither; np.array_equal, so that -0.0 = +0.0.  The
    kernel acts value by value on ``count`` doubles and reads nothing of the registered mesh: the context of either node
    order must give the same values."""
    hp, _ = _mods()
    lo_, hi_ = box
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, 5, order)
    rng = np.random.default_rng(7)
    s0 = 0.75
    try:
        for count in COUNTS:
            g = rng.standard_normal(count)
            gd, cB, sB = ctx.array(g), ctx.empty(16 * count), ctx.empty(16 * count)
            for alpha in ALPHAS:
                c, d = _planted(rng, count, alpha, lo_, hi_)
                cd, dd = ctx.array(c), ctx.array(d)
                for K in (1, 2, 10, 16):
                    ref = np.concatenate([po.prox_trial(c, s0 * (1 / 2 ** t), d, alpha, lo_, hi_) for t in range(K)])
                    assert ref.min() >= lo_ and ref.max() <= hi_
                    if K == 16 and count >= 12:
                        r = ref.reshape(K, count)
                        assert np.all(r[:, :2] == min(max(0.0, lo_), hi_)), "x = +-tau must give the clipped zero"
                        assert np.all(r[:, 6] == hi_) and np.all(r[:, 7] == lo_)
                    for with_g, with_src in ((True, True), (False, True), (False, False)):
                        cB.upload(np.full(16 * count, np.nan))
                        sB.upload(np.full(16 * count, np.nan))
                        ctx.prox_trials(cd, dd, s0, K, alpha, lo_, hi_, count, cB, sB if with_src else None,
                                        g=gd if with_g else None)
                        got, src = cB.download(), sB.download()
                        assert np.array_equal(got[:K * count], ref), (count, alpha, K, with_g, with_src)
                        assert np.all(np.isnan(got[K * count:]))
                        if with_src:
                            sref = 1.0 * np.tile(g, K) + 1.0 * ref if with_g else ref
                            assert np.array_equal(src[:K * count], sref), (count, alpha, K, with_g)
                            assert np.all(np.isnan(src[K * count:]))
                        else:
                            assert np.all(np.isnan(src))
                    if alpha == 0.0:
                        ctx.source_trials(cd, dd, s0, K, lo_, hi_, count, sB)
                        assert np.array_equal(sB.download()[:K * count], ref), (count, K)
                cd.free()
                dd.free()
            for a in (gd, cB, sB):
                a.free()
    finally:
        ctx.close()


def test_prox_trials_on_unaligned_blocks_and_more_than_one_grid_pass():
    """an even count whose pointers are 8 bytes off a 16-byte boundary (the scalar kernel), and 4096 * 256 * 2 + 6 values
    (more than one pass of the 16-byte kernel's grid)"""
    hp, _ = _mods()
    ctx = hp.Context(0)
    rng = np.random.default_rng(8)
    try:
        for count, off in ((1000, 1), (4096 * 256 * 2 + 6, 0)):
            c, d = rng.uniform(-1, 1, count + off), rng.standard_normal(count + off)
            cd, dd, cB = ctx.array(c), ctx.array(d), ctx.empty(2 * count + off)
            ctx.prox_trials(cd.ptr + 8 * off, dd.ptr + 8 * off, 1.0, 2, 0.05, -0.1, 0.5, count, cB.ptr + 8 * off)
            ref = np.concatenate([po.prox_trial(c[off:], s, d[off:], 0.05, -0.1, 0.5) for s in (1.0, 0.5)])
            assert np.array_equal(cB.download()[off:], ref)
            for a in (cd, dd, cB):
                a.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ l1_norm_Q, sparse_trial_stats
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nc", [5, 12, 40, 256])
def test_l1_norm_and_trial_stats(nc, order):
    """n = 36 (less than one wave), 169 (a ragged tail), 1681 (several blocks), 66 049 (four waves per block, the LDS
    stage of the tree); levels 1, 2, 8.

    l1_norm_Q, batch 1 and 3: within 1e-12 * value of NumPy (test_q_gram_matches_numpy's bar; every term is non-negative,
    so no cancellation), the same bits on a second call, and a trajectory of ones gives dt sum_l w_l sum_i ml_i.
    sparse_trial_stats, K = 1, 10, 16, on trials prox_trials wrote (a third to a half of the values exactly zero): dist
    bit-equal to l2_norm_sq_Q(c_t, c), l1 bit-equal to l1_norm_Q(c_t), nnz NumPy's count."""
    hp, _ = _mods()
    n, v2d, M, ml = _mesh(nc)
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, order)
    rng = np.random.default_rng(10 * nc + order)
    dt = 0.01
    try:
        for Nt in (0, 1, 7):
            tl = (Nt + 1) * n
            fields = [rng.standard_normal(tl) * 10.0 ** rng.integers(-3, 3) for _ in range(3)]
            fields[1][rng.random(tl) < 0.5] = 0.0
            a3 = ctx.array(np.concatenate([_to_dev(f, n, v2d, order) for f in fields]))
            ref = np.array([po.l1_norm_Q(f, Nt, dt, ml) for f in fields])
            for batch in (1, 3):
                got = ctx.l1_norm_Q(a3, Nt, dt, batch=batch)
                print(nc, order, Nt, batch, np.abs(got - ref[:batch]) / ref[:batch])
                assert got.shape == (batch,) and np.all(np.abs(got - ref[:batch]) <= 1e-12 * ref[:batch])
                assert ctx.l1_norm_Q(a3, Nt, dt, batch=batch).tobytes() == got.tobytes()
            ones = ctx.array(np.ones(tl))
            exact = dt * lo.q_weights(Nt).sum() * ml.sum()
            assert abs(ctx.l1_norm_Q(ones, Nt, dt)[0] - exact) <= 1e-12 * exact
            # trials around a reference control: the fused statistics against the primitives they fuse
            c, d = rng.uniform(-0.3, 0.6, tl), 0.3 * rng.standard_normal(tl)
            cd, dd, cB, ckB = ctx.array(c), ctx.array(d), ctx.empty(16 * tl), ctx.empty(16 * tl)
            for K in (1, 10, 16):
                ctx.prox_trials(cd, dd, 2.0, K, 0.25, -0.1, 0.5, tl, cB)
                for k in range(K):
                    ckB.copy_from(cd, tl, dst_off=k * tl)
                l1, dist, nnz = ctx.sparse_trial_stats(cB, cd, K, Nt, dt)
                assert l1.shape == dist.shape == nnz.shape == (K,) and nnz.dtype == np.int64
                assert dist.tobytes() == ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=K).tobytes(), (Nt, K)
                assert l1.tobytes() == ctx.l1_norm_Q(cB, Nt, dt, batch=K).tobytes(), (Nt, K)
                trials = cB.download()[:K * tl].reshape(K, tl)
                count = np.count_nonzero(trials, axis=1)
                assert np.array_equal(nnz, count), (Nt, K)
                assert 0 < count.min() and count[0] < 0.8 * tl
                assert ctx.sparse_trial_stats(cB, cd, K, Nt, dt)[0].tobytes() == l1.tobytes()
            for a in (a3, ones, cd, dd, cB, ckB):
                a.free()
    finally:
        ctx.close()


def test_scratch_that_grows_and_then_fits():
    """a long trajectory after a short one and a short one after it: each call sizes its own partials"""
    hp, _ = _mods()
    n, v2d, M, ml = _mesh(12)
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, 12, 1)
    rng = np.random.default_rng(3)
    try:
        for Nt in (1, 40, 3, 250, 0):
            tl = (Nt + 1) * n
            f = rng.standard_normal(2 * tl)
            a = ctx.array(f)
            ref = np.array([po.l1_norm_Q(f[:tl], Nt, 0.1, ml), po.l1_norm_Q(f[tl:], Nt, 0.1, ml)])
            assert np.all(np.abs(ctx.l1_norm_Q(a, Nt, 0.1, batch=2) - ref) <= 1e-12 * ref)
            l1, dist, nnz = ctx.sparse_trial_stats(a, a, 2, Nt, 0.1)
            assert np.all(np.abs(l1 - ref) <= 1e-12 * ref) and dist[0] == 0.0 and list(nnz) == [tl, tl]
            a.free()
    finally:
        ctx.close()


def test_primitives_reject_bad_arguments():
    hp, _ = _mods()
    ctx = hp.Context(0)
    try:
        a, out = ctx.zeros(32), ctx.zeros(16 * 32)
        with pytest.raises(hp.FemFctValueError):
            ctx.l1_norm_Q(a, 0, 1.0)                                    # no mass matrix
        with pytest.raises(hp.FemFctValueError):
            ctx.sparse_trial_stats(out, a, 1, 0, 1.0)
        ctx.set_mesh_square(-1, 1, 1, 1)                                # n = 4
        ok = dict(c=a, d=a, s0=1.0, K=2, alpha=1e-3, c_lower=-0.1, c_upper=0.5, count=32, c_out=out)
        ctx.prox_trials(**ok)
        for bad in (dict(alpha=-1e-300), dict(K=0), dict(K=17), dict(K=-1), dict(count=0), dict(count=-3),
                    dict(c_lower=0.5, c_upper=-0.1), dict(c=None), dict(d=None), dict(c_out=None)):
            with pytest.raises(hp.FemFctValueError):
                ctx.prox_trials(**dict(ok, **bad))
        ctx.prox_trials(**dict(ok, c_lower=0.2, c_upper=0.2))           # lo == hi is a box
        assert np.array_equal(out.download()[:64], np.full(64, 0.2))
        assert ctx.l1_norm_Q(a, 7, 1.0).shape == (1,)
        for bad in (dict(a=None), dict(num_steps=-1), dict(batch=0)):
            with pytest.raises(hp.FemFctValueError):
                ctx.l1_norm_Q(**dict(dict(a=a, num_steps=7, dt=1.0, batch=1), **bad))
        for bad in (dict(c_trials=None), dict(c_ref=None), dict(K=0), dict(K=17), dict(num_steps=-1)):
            with pytest.raises(hp.FemFctValueError):
                ctx.sparse_trial_stats(**dict(dict(c_trials=out, c_ref=a, K=2, num_steps=7, dt=1.0), **bad))
        assert ctx.sparse_trial_stats(out, a, 2, 7, 1.0)[2].tolist() == [32, 32]        # still usable
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ loops against the oracle
def _assert_same_run(dev, ora, tl):
    """_assert_same_run's bars of test_gpu_lbfgs.py: the same decisions, costs to 1e-9 relative, iterates, state and
    adjoint to 1e-8, every Armijo decision of both sides at least 1e-7 from its threshold; and for the sparse control, final
    supports that differ in at most 2 values (the oracle alone differs in 0 under a 1e-12 perturbation of u0) and
    nonzero fractions to 6e-4 (two values of 3549)"""
    (u, p, c, h), (uo, po_, co, ho) = dev, ora
    print("device", h["cost"], h["armijo_k"], h["nonzero_fraction"], h["armijo_margin_min"])
    print("oracle", ho["cost"], ho["armijo_k"], ho["nonzero_fraction"], ho["armijo_margin_min"])
    assert h["armijo_k"] == ho["armijo_k"] and h["sweeps"] == ho["sweeps"] and not h["stalled"] and not ho["stalled"]
    assert h["step"] == ho["step"] and h["iterations"] == ho["iterations"] == len(ho["cost"])
    assert np.allclose(h["cost"], ho["cost"], rtol=1e-9, atol=0)
    assert np.allclose(h["cost_smooth"], ho["cost_smooth"], rtol=1e-9, atol=0)
    assert np.allclose(h["l1"], ho["l1"], rtol=1e-9, atol=0)
    # the residual is the squared Q norm of prox(c - g) - c, a difference whose norm falls to 4.7e-4 of ||c||_Q in these
    # runs (CPU figures): fields that agree to 1e-8 of their norm move it by up to 2 * 3e-8 / 4.7e-4 = 1.3e-4 relative
    print("residual", np.abs(np.array(h["residual"]) / np.array(ho["residual"]) - 1))
    assert np.allclose(h["residual"], ho["residual"], rtol=1e-3, atol=0)
    assert abs(h["cost0"] - ho["cost0"]) <= 1e-9 * abs(ho["cost0"])
    assert ho["armijo_margin_min"] > 1e-7 and h["armijo_margin_min"] > 1e-7
    assert [len(m) for m in h["armijo_margin"]] == [len(m) for m in ho["armijo_margin"]]
    assert _rel(c, co) < 1e-8 and _rel(u, uo) < 1e-8 and _rel(p, po_) < 1e-8
    assert np.count_nonzero((c != 0) != (co != 0)) <= 2
    assert np.allclose(h["nonzero_fraction"], ho["nonzero_fraction"], rtol=0, atol=6e-4)
    assert h["nonzero_fraction"][-1] == np.count_nonzero(c) / tl
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


@functools.lru_cache(maxsize=None)
def _drift_case():
    return po.drift_case()


def _device_drift(cs, alpha, iters, starts=None, **kw):
    hp, solvers = _mods()
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    ct = None if starts is None else solvers.ControlIntervals(cs["Nt"], list(starts))
    try:
        return solvers.prox_solidbody(prob, cs["u0"], cs["uhat"], cs["c0"], cs["beta"], alpha, cs["lo"], cs["hi"], iters,
                                      optim=cs["optim"], control_time=ct, **kw)
    finally:
        prob.close()


@pytest.mark.parametrize("alpha", [1e-4, 5e-4])
def test_prox_solidbody_matches_oracle_loop(alpha):
    """13 x 13 nodes, 20 steps, target from the control that is 2 on levels 0..10 and 0 after, c0 = 0, s0 = 256, eight
    iterations.  On the CPU: armijo_k [1,3,1,4,1,2,3,2] / [1,3,1,4,1,1,2,3], final nonzero fraction 0.320 / 0.194, every
    Armijo decision at least 9.0e-3 / 1.4e-2 from its threshold; both signs and both bounds occur."""
    cs = _drift_case()
    ora = po.run_solidbody(cs, po.DRIFT_ITERS, alpha, s0=po.DRIFT_S0)
    dev = _device_drift(cs, alpha, po.DRIFT_ITERS, s0=po.DRIFT_S0)
    assert ora[3]["armijo_k"] == po.DRIFT_ARMIJO_K[alpha]
    _assert_same_run(dev, ora, cs["tl"])
    c = dev[2]
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]
    assert np.any(c == cs["lo"]) and np.any(c == cs["hi"]) and np.any((c < 0) & (c > cs["lo"])) and np.any(c > 0)
    assert dev[3]["nonzero_fraction"][-1] < 0.35


def test_piecewise_constant_sparse_controls_stay_piecewise_constant_bitwise():
    """ControlIntervals(Nt, [0, 7, 21]) on the drift case: c and g are constant on every interval and the prox acts value
    by value, so every iterate is, bit for bit; and the run is the reference loop's with the projected direction"""
    _, solvers = _mods()
    cs, starts = _drift_case(), (0, 7, 21)
    dev = _device_drift(cs, 1e-4, po.DRIFT_ITERS, starts=starts, s0=po.DRIFT_S0)
    assert solvers.ControlIntervals(cs["Nt"], list(starts)).contains(dev[2], cs["n"])
    assert not np.array_equal(dev[2], cs["c0"])
    _assert_same_run(dev, po.run_solidbody(cs, po.DRIFT_ITERS, 1e-4, s0=po.DRIFT_S0, starts=starts), cs["tl"])


def test_alpha_zero_is_projected_gradient_with_this_search():
    """configuration A-finaltime, six iterations: lbfgs_solidbody(memory=0, speculative=True)'s decisions, its costs and
    iterates to 1e-11 (test_speculative_equals_sequential's bar)"""
    hp, solvers = _mods()
    cs = lo.solidbody_case(*lo.CONFIGS["A-finaltime"])
    u, p, c, h = _device_drift(cs, 0.0, 6)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    try:
        ul, pl, cl, hl = solvers.lbfgs_solidbody(prob, cs["u0"], cs["uhat"], cs["c0"], cs["beta"], cs["lo"], cs["hi"], 6,
                                                 memory=0, speculative=True, optim=cs["optim"])
    finally:
        prob.close()
    assert h["armijo_k"] == hl["armijo_k"] and h["sweeps"] == hl["sweeps"] and len(h["cost"]) == 6
    assert np.allclose(h["cost"], hl["cost"], rtol=1e-11, atol=0) and np.allclose(h["cost_smooth"], hl["cost"], rtol=1e-11)
    assert _rel(c, cl) < 1e-11 and _rel(u, ul) < 1e-11 and _rel(p, pl) < 1e-11


def _device_source(cs, alpha, s0, iters, c0=None, **kw):
    hp, solvers = _mods()
    from oracle import traj as otraj
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, cs["nc"]), cs["Nt"], cs["dt"], otraj.exact_velocity, eps=1e-3)
    try:
        return solvers.prox_source_control(prob, cs["u0"], cs["uhat"], cs["c0"] if c0 is None else c0, cs["beta"], alpha,
                                           cs["lo"], cs["hi"], g=cs["g"], optim="alltime", s0=s0, max_iters=iters, **kw)
    finally:
        prob.close()


@pytest.mark.parametrize("run", sorted(po.SOURCE_RUNS))
def test_prox_source_control_matches_oracle_loop(run):
    """n = 49, 18 steps, dt = 1/36, box [-0.1, 0.5], c0 = 0.08 cos(3 pi x) cos(2 pi y).  On the CPU: alpha = 1e-2, s0 = 1024,
    eight iterations: armijo_k [1,3,1,3,1,3,1,4], final F 5.4184e-3, every Armijo decision at least 1.1e-4 from its
    threshold, 14 % of the final values at -0.1, 34 % at 0.5, 52 % nonzero; alpha = 3e-3, s0 = 64, six iterations:
    armijo_k [1,1,1,2,2,3], 5.2e-4."""
    alpha, s0, iters = run
    cs = po.source_case()
    ora = po.run_source(cs, iters, alpha, s0)
    assert ora[3]["armijo_k"] == po.SOURCE_RUNS[run]
    dev = _device_source(cs, alpha, s0, iters)
    _assert_same_run(dev, ora, cs["tl"])
    c = dev[2]
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"] and np.any(c == cs["hi"]) and np.any(c == 0)
    if alpha == 1e-2:
        assert np.any(c == cs["lo"]) and abs(dev[3]["cost"][-1] - 5.4184e-3) < 1e-7


def test_a_search_without_an_acceptable_trial_stalls_and_keeps_the_control():
    """one trial of step 1e6 per iteration, started from the bang-bang control at which the reference loop stalls: no
    trial passes, ``stalled`` is set, the control comes back unchanged and nothing is raised"""
    cs = po.source_case()
    start = po.run_source(cs, 3, 1e-2, 1e6, max_armijo=1)[2]
    u, p, c, h = _device_source(cs, 1e-2, 1e6, 3, c0=start, max_armijo=1)
    assert h["stalled"] and h["iterations"] == 0 and h["cost"] == [] and h["armijo_margin_min"] is None
    assert np.array_equal(c, start) and np.isfinite(h["cost0"])


def test_loops_reject_bad_arguments():
    hp, solvers = _mods()
    cs = _drift_case()
    for bad in (dict(alpha=-1.0), dict(max_armijo=0), dict(max_armijo=17)):
        with pytest.raises(ValueError):
            _device_drift(cs, bad.pop("alpha", 1e-4), 1, **bad)
    with pytest.raises(ValueError):
        _device_drift(dict(cs, c0=cs["c0"][:-1]), 1e-4, 1)
    with pytest.raises(ValueError):
        _device_drift(dict(cs, lo=1.0, hi=0.0), 1e-4, 1)


def test_example_runs():
    """examples/sparse_source_control_pdeco.py, two iterations for both values of alpha, as a child process"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "sparse_source_control_pdeco.py"), "--iters", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.count("proximal gradient, alpha") == 2 and out.stdout.count("\n   2  ") == 2, out.stdout
