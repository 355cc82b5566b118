"""GPU tests of the low-order operator built for every level before a sweep (FEMFCT_PREBUILD_LOW, -m gpu).

L_k = M_L + dt (A_k - D_k) and D_k depend on the control only; in the latency regime (81 x 81 mesh, one trajectory) they
are built next to the pre-assembled A_k sequence, and the first Jacobi launch and the fused limiter of every step read
them instead of building them.  The expressions are those of the in-launch build: every bit must stay the same."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NC, DT, OM = 80, 1e-3, np.pi / 40      # C2 / C5: [-1, 1]^2, 81 x 81 nodes, dt = 1e-3


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


def c2_inputs(hp, Nt, c5):
    """(u0, control, target) in the device's vertex order: slotted disc and a smooth space-time control (C2), or a
    Gaussian and c = 1 (C5), as bench.py sets them up."""
    mesh = hp.SquareMeshP1(-1, 1, NC)
    n = mesh.nodes
    x, y = mesh.coordinates()       # vertex order
    if c5:
        u0 = np.exp(-20 * ((x + 2 / 3) ** 2 + 5 * (y + 5 / 6) ** 2))
        c = np.ones((Nt + 1) * n)
    else:
        R = np.sqrt(x ** 2 + (y - 1 / 3) ** 2)
        u0 = ((R < 1 / 3) & ((np.abs(x) > 0.05) | (y > 0.5))).astype(np.float64)
        t = np.linspace(0.0, 1.0, Nt + 1)[:, None]
        c = np.clip(1.5 + np.sin(2 * np.pi * (x[None, :] + t)) * np.cos(np.pi * y[None, :]) + 0.5 * t, 0.0, 5.0).reshape(-1)
    uhat = np.roll(u0, 7)
    return mesh, u0, c, uhat


def run(hp, solvers, monkeypatch, prebuild, graphs, Nt, c5):
    monkeypatch.setenv("FEMFCT_PREBUILD_LOW", prebuild)
    mesh, u0, c, uhat = c2_inputs(hp, Nt, c5)
    n = mesh.nodes
    optim = "alltime" if c5 else "finaltime"
    prob = solvers.SolidBodyDrift(mesh, Nt, DT, om=OM, rot_scale=0.0 if c5 else 1.0, order=hp.ORDER_VERTEX)
    try:
        ctx = prob.ctx
        ctx.set_graphs(graphs)
        assert ctx.kernel_regime(1) == hp._lib.REGIME_TILE32
        tl = (Nt + 1) * n
        init = np.zeros(tl)
        init[:n] = u0
        d_c, d_u = ctx.array(c), ctx.array(init)
        d_uhat = ctx.array(np.tile(uhat, Nt + 1) if c5 else uhat)
        d_p, d_d = ctx.zeros(tl), ctx.zeros(tl)
        for _ in range(2):                  # the second sweep of each kind runs at the settled budget
            prob.forward(d_c, d_u, batch=1)
        logf = {k: v.copy() for k, v in prob.solver_log(1).items()}
        for _ in range(2):
            prob.adjoint(d_c, d_u, d_uhat, d_p, optim, batch=1)
        loga = {k: v.copy() for k, v in prob.solver_log(1).items()}
        prob.descent_direction(d_c, d_u, d_p, 1.0, d_d)
        res = dict(u=d_u.download(), p=d_p.download(), d=d_d.download(), logf=logf, loga=loga, c=c, u0=u0, uhat=uhat)
        # launches of the "assemble" class in one forward sweep: the A_k sequence, and the L_k / D_k one when pre-built
        ctx.set_profiling(True)
        prob.forward(d_c, d_u, batch=1)
        res["assembles"] = ctx.profile_report()["assemble"][1]
        ctx.set_profiling(False)
        return res
    finally:
        prob.close()


def assert_same_bits(a, b):
    for k in ("u", "p", "d"):
        assert np.array_equal(a[k], b[k]), k
    for la, lb in ((a["logf"], b["logf"]), (a["loga"], b["loga"])):
        for k in la:
            assert np.array_equal(la[k], lb[k]), k


@pytest.mark.parametrize("c5", [False, True], ids=["c2", "c5"])
def test_prebuilt_low_order_operator_is_bitwise_neutral(hp, solvers, monkeypatch, c5):
    """C2 (250 + 250 steps, final-time misfit) and the C5 set-up (100 + 100, all-time misfit, no rotation): trajectories,
    per-step solver records and descent direction with the pre-built L_k / D_k equal those of the in-launch build to the
    bit, with graphs on and off; the pre-built sequence is really built (one more assemble launch per sweep)."""
    Nt = 100 if c5 else 250
    on = run(hp, solvers, monkeypatch, "1", True, Nt, c5)
    off = run(hp, solvers, monkeypatch, "0", True, Nt, c5)
    eager = run(hp, solvers, monkeypatch, "1", False, Nt, c5)
    assert on["assembles"] == 2 and off["assembles"] == 1, (on["assembles"], off["assembles"])
    assert np.abs(on["u"]).max() > 0 and np.abs(on["p"]).max() > 0
    assert_same_bits(on, off)
    assert_same_bits(on, eager)


def test_prebuilt_low_order_operator_c2_vs_oracle(hp, solvers, monkeypatch):
    """The whole C2 sweep pair with the pre-built operator against the CPU oracle (2.6e-13 / 9e-13 expected)."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    Nt = 250
    res = run(hp, solvers, monkeypatch, "1", True, Nt, False)
    omesh = SquareMesh(-1, 1, NC)
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
    assert rel(to_dof(res["u"]), uk) < 1e-10
    assert rel(to_dof(res["p"]), pk) < 1e-10
