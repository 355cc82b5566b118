"""GPU tests of the hexagonal cone and of the fitted patches of the tile kernels (FEMFCT_TILE_CONE, FEMFCT_TILE_FIT, -m gpu).

With FEMFCT_TILE_CONE=1 the lean loops of kernels_tile32.hip take a node's liveness from the graph distance of the P1
stencil (a hexagon) instead of the max-norm, and a thread loads its matrix row only where the node is ever live and
its iterate only where a live node reads it.  With FEMFCT_TILE_FIT=1 the fused du/dt and limiter launches run 6 x 6
tiles on patches of 26 and 30 nodes per side while every workgroup gets a compute unit.  Each knob at 0 is the code as
it was.  Operands and their order are the same for every owned node: every bit of the trajectories, of the per-step
solver records and of the descent direction must be."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, OM = 1e-3, np.pi / 40
NT = 12                                 # steps per sweep: 12 forward + 12 adjoint


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def inputs(hp, N, Nt, c5, batch):
    """(u0, controls, target) in vertex order: slotted disc and a smooth space-time control (C2), or a Gaussian and
    c = 1 (C5), as bench.py sets them up; member m of a batch gets its own phase and amplitude."""
    mesh = hp.SquareMeshP1(-1, 1, N - 1)
    x, y = mesh.coordinates()
    if c5:
        u0 = np.exp(-20 * ((x + 2 / 3) ** 2 + 5 * (y + 5 / 6) ** 2))
    else:
        R = np.sqrt(x ** 2 + (y - 1 / 3) ** 2)
        u0 = ((R < 1 / 3) & ((np.abs(x) > 0.05) | (y > 0.5))).astype(np.float64)
    t = np.linspace(0.0, 1.0, Nt + 1)[:, None]
    cs = []
    for m in range(batch):
        if c5 and batch == 1:
            cs.append(np.ones((Nt + 1) * mesh.nodes))
        else:
            cs.append(np.clip(1.5 + (1.0 - 0.2 * m) * np.sin(2 * np.pi * (x[None, :] + t + 0.3 * m)) * np.cos(np.pi * y[None, :])
                              + 0.5 * t, 0.0, 5.0).reshape(-1))
    return mesh, u0, np.stack(cs), np.roll(u0, 7)


def run(hp, solvers, monkeypatch, cone, fit, N=81, Nt=NT, c5=False, batch=1, graphs=True, eps=0.0, env=None, u0_poison=None):
    monkeypatch.setenv("FEMFCT_TILE_CONE", cone)
    monkeypatch.setenv("FEMFCT_TILE_FIT", fit)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    mesh, u0, c, uhat = inputs(hp, N, Nt, c5, batch)
    n = mesh.nodes
    alltime = c5 or batch > 1
    prob = solvers.SolidBodyDrift(mesh, Nt, DT, om=OM, eps=eps, rot_scale=0.0 if c5 else 1.0, batch=batch,
                                  order=hp.ORDER_VERTEX)
    try:
        ctx = prob.ctx
        ctx.set_graphs(graphs)
        assert ctx.kernel_regime(batch) == hp._lib.REGIME_TILE32
        tl = (Nt + 1) * n
        init = np.zeros((batch, tl))
        init[:, :n] = u0
        if u0_poison is not None:
            init[0, u0_poison] = np.nan
        d_c, d_u = ctx.array(c.ravel()), ctx.array(init.ravel())
        d_uhat = ctx.array(np.tile(uhat, batch * (Nt + 1)) if alltime else uhat)
        d_p, d_d = ctx.zeros(batch * tl), ctx.zeros(tl)
        for _ in range(2):                  # the second sweep of each kind runs at the settled budget
            prob.forward(d_c, d_u, batch=batch)
        logf = {k: v.copy() for k, v in prob.solver_log(batch).items()}
        for _ in range(2):
            prob.adjoint(d_c, d_u, d_uhat, d_p, "alltime" if alltime else "finaltime", batch=batch)
        loga = {k: v.copy() for k, v in prob.solver_log(batch).items()}
        if batch == 1:                      # (the direction is a single-trajectory call)
            prob.descent_direction(d_c, d_u, d_p, 1.0, d_d)
        return dict(u=d_u.download(), p=d_p.download(), d=d_d.download(), logf=logf, loga=loga, c=c[0], u0=u0, uhat=uhat)
    finally:
        prob.close()


def assert_same_bits(a, b):
    for k in ("u", "p", "d"):
        assert np.array_equal(a[k], b[k]), k
    for la, lb in ((a["logf"], b["logf"]), (a["loga"], b["loga"])):
        for k in la:
            assert np.array_equal(la[k], lb[k]), k


def assert_knobs_are_neutral(hp, solvers, monkeypatch, **kw):
    """Both knobs on, each knob alone, against both off."""
    off = run(hp, solvers, monkeypatch, "0", "0", **kw)
    assert np.abs(off["u"]).max() > 0 and np.abs(off["p"]).max() > 0
    assert np.isfinite(off["u"]).all() and np.isfinite(off["p"]).all()
    for cone, fit in (("1", "1"), ("1", "0"), ("0", "1")):
        assert_same_bits(run(hp, solvers, monkeypatch, cone, fit, **kw), off)


@pytest.mark.parametrize("c5", [False, True], ids=["c2-finaltime", "c5-alltime"])
def test_flagship_kernels(hp, solvers, monkeypatch, c5):
    """N = 81, one trajectory: H = 13 Jacobi launches on the cone, 14 x 15 and 14 x 14 workgroups on the fitted patches."""
    assert_knobs_are_neutral(hp, solvers, monkeypatch, c5=c5)


@pytest.mark.parametrize("N", [46, 48, 47])
def test_fitted_patch_edge_on_the_mesh_edge(hp, solvers, monkeypatch, N):
    """N = 6 b + 16: the last 26-patch (du/dt launch) ends exactly on the mesh edge; N = 6 b + 18: the last 30-patch
    (limiter launch); N = 47: neither.  Edge lanes are then inside the mesh, exact for every sweep, and read clamped
    neighbours."""
    assert ((N - 16) % 6 == 0, (N - 18) % 6 == 0) == {46: (True, False), 48: (False, True), 47: (False, False)}[N]
    assert_knobs_are_neutral(hp, solvers, monkeypatch, N=N, env={"FEMFCT_MESH_STEP": "0"})


def test_fitted_patches_with_a_batch(hp, solvers, monkeypatch):
    """N = 43, two trajectories: 8 x 9 x 2 workgroups fit the compute units, the fitted geometry runs with blockIdx.z."""
    assert 8 * 9 * 2 <= 256
    assert_knobs_are_neutral(hp, solvers, monkeypatch, N=43, batch=2, env={"FEMFCT_MESH_STEP": "0"})


def test_batch_falls_back_to_the_32_patches(hp, solvers, monkeypatch):
    """N = 81, two trajectories: 14 x 15 x 2 > 256 workgroups, so the fused launches keep T = 12 and T = 8 and the cone
    loads run on the 32-patches."""
    assert 14 * 15 * 2 > 256
    assert_knobs_are_neutral(hp, solvers, monkeypatch, batch=2)


def test_full_rows(hp, solvers, monkeypatch):
    """eps = 1e-3: diffusion fills every off-diagonal of the operator and L is not an upwind matrix (no exact zeros)."""
    assert_knobs_are_neutral(hp, solvers, monkeypatch, eps=1e-3)


@pytest.mark.parametrize("knobs", ["1", "0"], ids=["on", "off"])
def test_nan_in_the_nw_corner_fails_the_solve(hp, solvers, monkeypatch, knobs):
    """A NaN in u0 at the NW corner node of the mesh -- outside the cone of most patches -- still ends in NotConverged
    (as tests/test_gpu_nonfinite.py expects of this regime): the patches that own it and its neighbours load it."""
    with pytest.raises(hp.NotConverged):
        run(hp, solvers, monkeypatch, knobs, knobs, Nt=4, u0_poison=81 * 80)
