"""GPU tests of the lean sweep loops of the 32 x 32 tile kernels (FEMFCT_TILE_LEAN, -m gpu).

With FEMFCT_TILE_LEAN=1 (the default) the Jacobi and Chebyshev loops of kernels_tile32.hip keep the node's own value in
a register, address two static LDS buffers and update a node only while the owned tile can still see the result;
FEMFCT_TILE_LEAN=0 runs the loops as they were.  Operands and their order are the same: every bit of the trajectories,
of the per-step solver records and of the descent direction must be."""
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


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


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


def run(hp, solvers, monkeypatch, lean, N=81, Nt=NT, c5=False, batch=1, graphs=True, eps=0.0, env=None, u0_poison=None):
    monkeypatch.setenv("FEMFCT_TILE_LEAN", lean)
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


def assert_lean_is_neutral(hp, solvers, monkeypatch, **kw):
    on = run(hp, solvers, monkeypatch, "1", **kw)
    off = run(hp, solvers, monkeypatch, "0", **kw)
    assert np.abs(on["u"]).max() > 0 and np.abs(on["p"]).max() > 0
    assert np.isfinite(on["u"]).all() and np.isfinite(on["p"]).all()
    assert_same_bits(on, off)


@pytest.mark.parametrize("c5", [False, True], ids=["c2-finaltime", "c5-alltime"])
def test_flagship_kernels(hp, solvers, monkeypatch, c5):
    """N = 81, one trajectory: H = 13, two Jacobi launches, deferred residual test, fused du/dt and limiter launches."""
    assert_lean_is_neutral(hp, solvers, monkeypatch, c5=c5)


@pytest.mark.parametrize("N,H", [(43, 13), (46, 10), (44, 12)])
def test_patch_edge_on_the_mesh_edge(hp, solvers, monkeypatch, N, H):
    """N = 6 b + 19, 12 b + 22, 8 b + 20: the last patch of halo 13, 10, 12 ends exactly on the mesh edge, so its edge
    lanes are inside the mesh, exact for every sweep, and read clamped neighbours.  (Halo 13: the Jacobi launches by
    FEMFCT_STRIP_K; 10 and 12 are the halos of the fused du/dt and limiter launches, which all three cases run.)"""
    env = {"FEMFCT_MESH_STEP": "0", "FEMFCT_STRIP_K": str(H)}
    assert (N - (32 - H)) % (32 - 2 * H) == 0
    assert_lean_is_neutral(hp, solvers, monkeypatch, N=N, env=env)


@pytest.mark.parametrize("env", [
    {"FEMFCT_STRIP_K": "8"},
    {"FEMFCT_STRIP_K": "11"},
    {"FEMFCT_STRIP_K": "8", "FEMFCT_DEFER_CHECK": "0", "FEMFCT_EXACT": "1"},
    {"FEMFCT_STRIP_K": "11", "FEMFCT_DEFER_CHECK": "0", "FEMFCT_EXACT": "1"},
    {"FEMFCT_DEFER_CHECK": "0"},
    {"FEMFCT_EXACT": "1"},
    {"FEMFCT_FUSE_FLUX": "0", "FEMFCT_FUSE_DUDT": "0"},
    {"FEMFCT_FUSE_FLUX": "0"},
    {"FEMFCT_PREBUILD_LOW": "0"},
], ids=lambda e: "-".join(f"{k[7:].lower()}{v}" for k, v in e.items()))
def test_other_launch_variants(hp, solvers, monkeypatch, env):
    """Even and odd sweep counts per launch (the odd tail of the loop unrolled by two), the in-launch residual test,
    the per-sweep residual log of the last launch, the plain k_tile_cheb chain, the operator built in launch 0."""
    assert_lean_is_neutral(hp, solvers, monkeypatch, env=env)


def test_batch_of_three_controls(hp, solvers, monkeypatch):
    """Three trajectories with three different controls in one launch (blockIdx.z offsets), all-time misfit."""
    assert_lean_is_neutral(hp, solvers, monkeypatch, batch=3)


def test_full_rows(hp, solvers, monkeypatch):
    """eps = 1e-3: diffusion fills every off-diagonal of the operator (no exact zeros in L)."""
    assert_lean_is_neutral(hp, solvers, monkeypatch, eps=1e-3)


def test_eager_enqueue(hp, solvers, monkeypatch):
    assert_lean_is_neutral(hp, solvers, monkeypatch, graphs=False)


def test_lean_c2_vs_oracle(hp, solvers, monkeypatch):
    """25 + 25 steps of C2 with the lean loops against the CPU oracle."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    Nt = 25
    res = run(hp, solvers, monkeypatch, "1", Nt=Nt)
    omesh = SquareMesh(-1, 1, 80)
    n = omesh.nodes
    v2d = omesh.vertex_to_dof

    def to_dof(x):              # vertex order -> the oracle's DoF order
        out = np.empty_like(x.reshape(-1, n))
        out[:, v2d] = x.reshape(-1, n)
        return out.reshape(-1)

    sb = otraj.SolidBody(P1Assembler(omesh), om=OM)
    ck = to_dof(res["c"])
    uk = np.zeros((Nt + 1) * n)
    uk[:n] = to_dof(res["u0"])
    otraj.solidbody_forward(sb, ck, uk, n, Nt, DT)
    pk = otraj.solidbody_adjoint(sb, ck, uk, to_dof(res["uhat"]), np.zeros_like(uk), n, Nt, DT)
    eu, ep = rel(to_dof(res["u"]), uk), rel(to_dof(res["p"]), pk)
    print(f"[tile lean] C2 25 + 25 steps vs oracle: u {eu:.2e}, p {ep:.2e}")
    assert eu < 1e-10
    assert ep < 1e-10


@pytest.mark.parametrize("where", ["interior", "corner"])
def test_nan_in_u0_fails_the_solve(hp, solvers, monkeypatch, where):
    """A NaN in the initial state still ends in NotConverged (as tests/test_gpu_nonfinite.py expects of this regime):
    the residual maximum of the owned nodes is taken by nan_max in the lean loops too."""
    node = 81 * 47 + 30 if where == "interior" else 0
    with pytest.raises(hp.NotConverged):
        run(hp, solvers, monkeypatch, "1", Nt=4, u0_poison=node)
