"""Projected L-BFGS on the device (solvers.lbfgs_solidbody, solvers.lbfgs_source_control, solvers.LimitedMemory): the
three primitives femfct_free_set / femfct_q_gram / femfct_q_combine against NumPy, and the loops against the CPU
reference loop (lbfgs_oracle.py) on the configurations test_lbfgs_oracle.py checks on the CPU."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lbfgs_oracle as lo

pytestmark = pytest.mark.gpu

ITERS = 6


def _mods():
    return importlib.import_module("fem-fct-pdeco_amd"), importlib.import_module("fem-fct-pdeco_amd.solvers")


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


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


# ------------------------------------------------------------------------------------------------------------ q_gram
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nc", [5, 12, 40])
def test_q_gram_matches_numpy(nc, order):
    """n = 36 (less than one wave), 169 (a ragged tail), 1681 (several blocks); num_steps 0, 1, 7; J = 1, 2, 11, 17 and a
    list with a repeated pointer; no mask, a random one, all bound.  |G_ij - ref| <= 1e-12 sqrt(G_ii G_jj): the sums have
    at most 7 * 8 * 1681 terms per row tree, four decades above f64 rounding and six below any indexing error."""
    hp, _ = _mods()
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    omesh = SquareMesh(-1, 1, nc)
    M = P1Assembler(omesh).mass()
    n, v2d = omesh.nodes, omesh.vertex_to_dof
    to_dev = lambda x: x if order == 1 else np.ascontiguousarray(x.reshape(-1, n)[:, v2d]).reshape(-1)
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, order)
    rng = np.random.default_rng(100 * nc + order)
    dt = 0.01
    try:
        for Nt in (0, 1, 7):
            tl = (Nt + 1) * n
            fields = [rng.standard_normal(tl) * 10.0 ** rng.integers(-3, 3) for _ in range(17)]
            dev = [ctx.array(to_dev(f)) for f in fields]
            masks = {"none": None, "random": rng.random(tl) > 0.4, "bound": np.zeros(tl, dtype=bool)}
            for name, mask in masks.items():
                md = None if mask is None else _bytes(ctx, hp, tl, to_dev(mask.astype(np.uint8)))
                for J in (1, 2, 11, 17):
                    G = ctx.q_gram(dev[:J], Nt, dt, mask=md)
                    assert G.shape == (J, J) and np.array_equal(G, G.T)
                    assert ctx.q_gram(dev[:J], Nt, dt, mask=md).tobytes() == G.tobytes()
                    if name == "bound":
                        assert np.array_equal(G, np.zeros((J, J)))
                        continue
                    ref = lo.q_gram(fields[:J], mask, Nt, dt, M)
                    bound = 1e-12 * np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
                    assert np.all(np.abs(G - ref) <= bound), (Nt, name, J, np.max(np.abs(G - ref) / bound))
                    if mask is None:
                        for i in range(J):
                            assert G[i, i].tobytes() == ctx.l2_norm_sq_Q(dev[i], None, Nt, dt)[0].tobytes(), (Nt, J, i)
                # one pointer twice
                G = ctx.q_gram([dev[0], dev[1], dev[0]], Nt, dt, mask=md)
                ref = lo.q_gram([fields[0], fields[1], fields[0]], mask, Nt, dt, M)
                assert np.all(np.abs(G - ref) <= 1e-12 * np.sqrt(np.outer(np.diag(ref), np.diag(ref))))
                assert G[0, 0] == G[2, 2] == G[0, 2]
                if md is not None:
                    md.free()
            for a in dev:
                a.free()
    finally:
        ctx.close()


def test_q_gram_four_waves_per_block_diagonal_is_the_norm():
    """n = 257^2 > 65536: blocks of four waves, the LDS stage of the tree; unmasked diagonal = l2_norm_sq_Q bit for bit,
    off-diagonal against NumPy"""
    hp, _ = _mods()
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    nc, Nt, dt = 256, 1, 0.01
    omesh = SquareMesh(-1, 1, nc)
    M = P1Assembler(omesh).mass()
    n = omesh.nodes
    ctx = hp.Context(0)
    ctx.set_mesh_square(-1, 1, nc, 1)
    rng = np.random.default_rng(5)
    try:
        fields = [rng.standard_normal((Nt + 1) * n) for _ in range(5)]
        dev = [ctx.array(f) for f in fields]
        G = ctx.q_gram(dev, Nt, dt)
        ref = lo.q_gram(fields, None, Nt, dt, M)
        assert np.all(np.abs(G - ref) <= 1e-12 * np.sqrt(np.outer(np.diag(ref), np.diag(ref))))
        for i in range(5):
            assert G[i, i].tobytes() == ctx.l2_norm_sq_Q(dev[i], None, Nt, dt)[0].tobytes()
    finally:
        ctx.close()


def test_primitives_reject_bad_arguments():
    hp, _ = _mods()
    ctx = hp.Context(0)
    try:
        a = ctx.zeros(8)
        with pytest.raises(ValueError):
            ctx.q_gram([a], 0, 1.0)                             # no mass matrix
        ctx.set_mesh_square(-1, 1, 1, 1)
        assert ctx.q_gram([a], 1, 1.0).shape == (1, 1)
        for bad in ([], [a] * 18, [a, None]):
            with pytest.raises(ValueError):
                ctx.q_gram(bad, 1, 1.0)
            with pytest.raises(ValueError):
                ctx.q_combine(bad, np.ones(len(bad)), 8, ctx.zeros(8))
        with pytest.raises(ValueError):
            ctx.q_combine([a], [1.0], 8, ctx.zeros(8), mask=ctx.zeros(1))      # a mask without a fallback
        with pytest.raises(ValueError):
            ctx.q_combine([a, a], [1.0], 8, ctx.zeros(8))
    finally:
        ctx.close()


# -------------------------------------------------------------------------------------------- free_set and q_combine
def test_free_set_equals_numpy_predicate_bitwise():
    hp, _ = _mods()
    ctx = hp.Context(0)
    lo_, hi_ = -0.25, 1.5
    rng = np.random.default_rng(2)
    try:
        count = 4096 * 256 + 70001                              # more than one pass of the grid, an odd tail
        c = rng.uniform(lo_ - 0.5, hi_ + 0.5, count)
        g = rng.standard_normal(count)
        c[:9] = [lo_, lo_, lo_, hi_, hi_, hi_, np.nextafter(lo_, 1), np.nextafter(hi_, 0), 0.3]
        g[:9] = [1.0, -1.0, 0.0, 1.0, -1.0, 0.0, 1.0, -1.0, 0.0]
        c[9:15] = [lo_, lo_, hi_, hi_, lo_, hi_]
        g[9:15] = [-0.0, 5e-324, -5e-324, 0.0, np.inf, -np.inf]
        cd, gd = ctx.array(c), ctx.array(g)
        mask = _bytes(ctx, hp, count)
        ctx.free_set(cd, gd, lo_, hi_, count, mask)
        got = _download_bytes(ctx, hp, mask, count)
        ref = lo.free_set(c, g, lo_, hi_).astype(np.uint8)
        assert np.array_equal(got, ref)
        assert list(got[:9]) == [0, 1, 1, 1, 0, 1, 1, 1, 1]
    finally:
        ctx.close()


@pytest.mark.parametrize("masked", [False, True])
def test_q_combine_equals_numpy_expression_bitwise(masked):
    hp, _ = _mods()
    ctx = hp.Context(0)
    rng = np.random.default_rng(3)
    count = 4096 * 256 + 77                                     # more than one pass of the grid, not a multiple of the block
    try:
        fields = [rng.standard_normal(count) * 10.0 ** rng.integers(-4, 4) for _ in range(17)]
        dev = [ctx.array(f) for f in fields]
        fb = rng.standard_normal(count)
        fbd, out = ctx.array(fb), ctx.empty(count)
        mask = rng.random(count) > 0.3 if masked else None
        md = _bytes(ctx, hp, count, mask.astype(np.uint8)) if masked else None
        for J in (1, 3, 17):
            coef = rng.standard_normal(J)
            ctx.q_combine(dev[:J], coef, count, out, mask=md, fallback=fbd if masked else None, fallback_scale=-1.0)
            ref = lo.combine(fields[:J], coef, mask, fb, -1.0)
            assert out.download().tobytes() == ref.tobytes(), J
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ loops against the oracle
@functools.lru_cache(maxsize=None)
def _case(name):
    return lo.solidbody_case(*lo.CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _oracle_run(name, memory=5, starts=None):
    u, p, c, h = lo.run_solidbody(_case(name), ITERS, memory, starts=starts)
    for a in (u, p, c):
        a.setflags(write=False)
    return u, p, c, h


@functools.lru_cache(maxsize=None)
def _device_run(name, speculative=True, starts=None):
    hp, solvers = _mods()
    cs = _case(name)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, cs["nc"]), cs["Nt"], cs["dt"], om=np.pi / 40)
    ct = None if starts is None else solvers.ControlIntervals(cs["Nt"], list(starts))
    try:
        return solvers.lbfgs_solidbody(prob, cs["u0"], cs["uhat"], cs["c0"], cs["beta"], cs["lo"], cs["hi"], ITERS, memory=5,
                                       speculative=speculative, optim=cs["optim"], control_time=ct)
    finally:
        prob.close()


def _assert_same_run(dev, ora):
    (u, p, c, h), (uo, po, co, ho) = dev, ora
    print("device", h["cost"], h["armijo_k"], h["used"], h["armijo_margin_min"])
    print("oracle", ho["cost"], ho["armijo_k"], ho["used"], ho["armijo_margin_min"])
    assert h["armijo_k"] == ho["armijo_k"] and h["used"] == ho["used"]
    assert h["pairs"] == ho["pairs"] and h["sweeps"] == ho["sweeps"] and not h["stalled"] and not ho["stalled"]
    assert np.allclose(h["cost"], ho["cost"], rtol=1e-9, atol=0)
    assert abs(h["cost0"] - ho["cost0"]) <= 1e-9 * abs(ho["cost0"])
    assert np.allclose(h["free_fraction"], ho["free_fraction"], rtol=0, atol=5e-4)      # (a value or two with g ~ 0)
    assert ho["armijo_margin_min"] > 1e-7 and h["armijo_margin_min"] > 1e-7
    assert [len(m) for m in h["armijo_margin"]] == [len(m) for m in ho["armijo_margin"]]
    assert _rel(c, co) < 1e-8 and _rel(u, uo) < 1e-8 and _rel(p, po) < 1e-8


@pytest.mark.parametrize("name", ["A", "B", "A-finaltime"])
def test_lbfgs_solidbody_matches_oracle_loop(name):
    """Six iterations with a memory of 5: the same decisions and directions taken, costs to 1e-9, iterates to 1e-8 (the
    tolerances of test_pgd_solidbody_matches_oracle_loop...: on the CPU a 1e-12 relative perturbation of u0 moves the
    costs by at most 3.9e-12 and the iterates by 6e-12, and every Armijo margin is at least 0.02 from its threshold).
    The sixth iteration of the final-time variant accepts its third trial."""
    dev, ora = _device_run(name), _oracle_run(name)
    _assert_same_run(dev, ora)
    h = dev[3]
    assert h["used"][0] == "g" and "qn" in h["used"]
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    if name == "A-finaltime":
        assert h["armijo_k"][-1] == 3
    if name == "B":
        assert min(h["free_fraction"]) < 1.0


def test_speculative_equals_sequential():
    (us, ps, cs_, hs), (uq, pq, cq, hq) = _device_run("A-finaltime", True), _device_run("A-finaltime", False)
    assert hs["armijo_k"] == hq["armijo_k"] and hs["used"] == hq["used"] and hs["sweeps"] == hq["sweeps"]
    assert max(hs["armijo_k"]) > 1
    assert _rel(cs_, cq) < 1e-11 and _rel(us, uq) < 1e-11 and np.allclose(hs["cost"], hq["cost"], rtol=1e-11, atol=0)


def test_iterates_stay_inside_the_box_exactly():
    cs = _case("B")
    c = _device_run("B")[2]
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]
    assert np.any(c == cs["lo"]) or np.any(c == cs["hi"])


def test_piecewise_constant_controls_stay_piecewise_constant_bitwise():
    """ControlIntervals(Nt, [0, 7, 21]) on configuration B: s, y, g and the free set are constant on every interval, so
    every iterate is, bit for bit; and the run is the reference loop's with the projected direction"""
    _, solvers = _mods()
    cs, starts = _case("B"), (0, 7, 21)
    dev = _device_run("B", True, starts)
    assert solvers.ControlIntervals(cs["Nt"], list(starts)).contains(dev[2], cs["n"])
    assert not np.array_equal(dev[2], cs["c0"]) and "qn" in dev[3]["used"]
    _assert_same_run(dev, _oracle_run("B", 5, starts))


def test_lbfgs_source_control_matches_oracle_loop_and_beats_projected_gradient():
    """The manufactured all-time problem on 10 x 10 cells (source_control_oracle.py's), five iterations: the reference
    loop's decisions, costs to 1e-9, and a cost below the one of memory = 0 (plain projected gradient with this search)"""
    hp, solvers = _mods()
    from oracle import traj as otraj
    cs = lo.source_case()
    uo, po, co, ho = lo.run_source(cs, 5, 5)
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(0.0, 1.0, cs["nc"]), cs["Nt"], cs["dt"], otraj.exact_velocity, eps=1e-3)
    try:
        run = lambda memory: solvers.lbfgs_source_control(prob, cs["u0"], cs["uhat"], cs["c0"], cs["beta"], cs["lo"], cs["hi"],
                                                          g=cs["g"], optim="alltime", memory=memory, max_iters=5, tol=0.0)
        u, p, c, h = run(5)
        h0 = run(0)[3]
    finally:
        prob.close()
    assert h["iterations"] == 5 and len(h["stop_crit"]) == len(h["stop_crit2"]) == 5
    _assert_same_run((u, p, c, h), (uo, po, co, ho))
    assert set(h0["used"]) == {"g"} and h0["pairs"] == [0] * 5
    print("memory 0", h0["cost"])
    assert h["cost"][-1] < h0["cost"][-1]
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]


def test_example_runs():
    """examples/lbfgs_solidbody_pdeco.py, two iterations of both loops on C2's problem, as a child process"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "lbfgs_solidbody_pdeco.py"), "--iters", "2"], capture_output=True,
                         text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "projected L-BFGS, memory 5" in out.stdout and "   2  " in out.stdout
