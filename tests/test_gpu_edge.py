"""Edge cases of the step operator through the C ABI (-m gpu): generic (non-mesh) sparsity patterns
with a different ELL width, tiny meshes, zero data, solver failure reporting."""
import importlib

import numpy as np
import pytest
from scipy.sparse import csr_matrix, diags

from regime_helpers import nine_point_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("N", [6, 23])
def test_generic_pattern_width_9(hp, N):
    from oracle import fct as ofct
    rng = np.random.default_rng(N)
    M, A = nine_point_problem(N, rng)
    n = N * N
    ml = np.asarray(M.sum(axis=1)).ravel()
    ML = diags(ml).tocsr()
    u_n = rng.random(n)
    rhs = 0.1 * rng.standard_normal(n)
    Nf = 0.05 * M
    dt = 0.02
    info = {}
    u = hp.FCT_alg_ref(A, rhs, u_n, dt, n, M, ML, None, non_flux_mat=Nf, info=info)
    uo = ofct.fct_step(A, rhs, u_n, dt, n, M, ML, None, non_flux_mat=Nf)
    assert rel(u, uo) < 1e-9, info
    y = hp.ChebSI(rhs, M, M.diagonal(), 7, 0.5, 2)
    assert rel(y, ofct.chebsi(rhs, M, M.diagonal(), 7, 0.5, 2)) < 1e-13


@pytest.mark.parametrize("nc", [1, 2, 3])
def test_tiny_meshes(hp, nc):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler, row_lump_diag
    from oracle import fct as ofct, traj as otraj
    mesh = SquareMesh(0, 1, nc)
    asm = P1Assembler(mesh)
    M = asm.mass()
    n = mesh.nodes
    ML = diags(row_lump_diag(M)).tocsr()
    rng = np.random.default_rng(nc)
    A = -(asm.convection(otraj.rotation_wind(3.0)) + asm.drift1(rng.random(n)))
    u_n = rng.random(n)
    u = hp.FCT_alg_ref(A, np.zeros(n), u_n, 1e-2, n, M, ML, None)
    assert rel(u, ofct.fct_step(A, np.zeros(n), u_n, 1e-2, n, M, ML, None)) < 1e-10
    # trajectories on the same tiny mesh, both DoF orders (tile kernels with a single, clipped patch)
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    Nt = 3
    sb = otraj.SolidBody(asm, om=3.0)
    ck = rng.random((Nt + 1) * n)
    uo = np.zeros((Nt + 1) * n); uo[:n] = u_n
    otraj.solidbody_forward(sb, ck, uo, n, Nt, 1e-2)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(0, 1, nc), Nt, 1e-2, om=3.0)
    ug = np.zeros((Nt + 1) * n); ug[:n] = u_n
    prob.solve_state(ck, ug)
    assert rel(ug, uo) < 1e-10
    prob.close()


def test_zero_state_and_zero_operator(hp):
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler, row_lump_diag
    asm = P1Assembler(SquareMesh(-1, 1, 8))
    M = asm.mass()
    n = M.shape[0]
    ML = diags(row_lump_diag(M)).tocsr()
    Z = csr_matrix((n, n))
    info = {}
    u = hp.FCT_alg_ref(Z, np.zeros(n), np.zeros(n), 1e-3, n, M, ML, None, info=info)
    assert np.array_equal(u, np.zeros(n)) and info["solver_resid"] == 0.0
    u1 = hp.FCT_alg_ref(Z, np.zeros(n), np.ones(n), 1e-3, n, M, ML, None)
    assert np.max(np.abs(u1 - 1.0)) < 1e-14          # zero operator: the state is kept


def test_solver_failure_is_reported_not_hidden(hp):
    """A sweep cap far below what the operator needs must raise, never return an unconverged state."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    from helpers_golden import load, fct_case
    c = fct_case(load("fct_cases.npz"), "rot_N41")
    Mc = c["M"].copy(); Mc.sort_indices()
    Ac = c["A"].copy(); Ac.sort_indices()
    for fusion in ((False, False), (True, False)):
        ctx = hp.Context(0)
        ctx.set_pattern_csr(Mc.indptr, Mc.indices)
        ctx.set_mass(Mc.data, c["ml"])
        ctx.set_fusion(*fusion)
        ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 4)
        with pytest.raises(hp.NotConverged):
            ctx.fct_step_host(Ac.data, c["rhs"], c["u_n"], c["dt"])
        ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 400)
        u, info = ctx.fct_step_host(Ac.data, c["rhs"], c["u_n"], c["dt"])
        assert rel(u, c["u_np1"]) < 1e-9 and not (info["flags"] & hp.FLAG_SOLVER_BUDGET)
        ctx.close()
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, 16), 4, 2e-3)
    prob.ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 3)
    n = prob.n
    uk = np.zeros(5 * n); uk[:n] = np.random.default_rng(0).random(n)
    with pytest.raises(hp.NotConverged):
        prob.solve_state(np.ones(5 * n), uk)
    prob.close()
    with pytest.raises(ValueError):
        hp.Context(0).set_solver(7, 1e-13, 10)


@pytest.mark.parametrize("name", ["rot_N41", "schnak_N41", "rotdrift22_bigdt_N41"])
def test_bicgstab_low_order_solver(hp, name):
    """femfct_set_solver(FEMFCT_SOLVER_BICGSTAB): same step through the Krylov low-order solve."""
    from helpers_golden import load, fct_case
    c = fct_case(load("fct_cases.npz"), name)
    pat = hp.fct_helpers._PatternCache.get_for(c["M"])     # values laid out on the pattern of M
    ctx = pat.ctx
    pat.set_mass(c["M"], c["ml"])
    ctx.set_solver(hp.SOLVER_BICGSTAB, 1e-13, 200)
    try:
        u, info = ctx.fct_step_host(pat.values(c["A"]), c["rhs"], c["u_n"], c["dt"],
                                    N_csr_vals=None if c["N"] is None else pat.values(c["N"]))
    finally:
        ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 400)
    assert rel(u, c["u_np1"]) < 1e-9, info
    assert bool(info["flags"] & hp.FLAG_MMATRIX_ROWSUM) == c["mmatrix_failed"]
    assert not (info["flags"] & hp.FLAG_SOLVER_BUDGET) and info["solver_iters"] > 0


def test_bicgstab_handles_a_time_step_jacobi_cannot(hp):
    """dt 40x beyond the scheme's CFL-type bound: Jacobi needs > 400 sweeps (reported), BiCGStab solves it;
    both are checked against the oracle's direct solve."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler, row_lump_diag
    from oracle import fct as ofct, traj as otraj
    mesh = SquareMesh(-1, 1, 24)
    asm = P1Assembler(mesh)
    M = asm.mass(); n = mesh.nodes
    ML = diags(row_lump_diag(M)).tocsr()
    A = -asm.convection(otraj.rotation_wind(np.pi / 40)) + 0.5 * asm.stiffness()
    rng = np.random.default_rng(5)
    u_n = rng.random(n)
    dt = 0.2
    uo = ofct.fct_step(A, np.zeros(n), u_n, dt, n, M, ML, None)
    pat = hp.fct_helpers._PatternCache.get_for(M)
    ctx = pat.ctx
    pat.set_mass(M, row_lump_diag(M))
    a = pat.values(A)
    try:
        ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 400)
        with pytest.raises(hp.NotConverged):
            ctx.fct_step_host(a, np.zeros(n), u_n, dt)
        ctx.set_solver(hp.SOLVER_BICGSTAB, 1e-13, 400)
        u, info = ctx.fct_step_host(a, np.zeros(n), u_n, dt)
    finally:
        ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 400)
    assert rel(u, uo) < 1e-9, info


def test_sweep_outside_the_dt_restriction_falls_back_to_bicgstab(hp, monkeypatch):
    """The reference's low-order solve is a direct one (spsolve, helpers.py:1782): it does not care whether the
    operator satisfies the scheme's dt restriction.  Jacobi does: at CFL ~ 8 its iteration matrix has spectral radius
    > 1.  The sweep must notice (no contraction after a whole budget), hand that KIND of sweep to BiCGStab, repeat it
    and deliver the reference result -- with the M-matrix diagnostic raised, as the reference prints "3: False"."""
    import importlib
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle import traj as otraj
    solvers = importlib.import_module("fem-fct-pdeco_amd.solvers")
    nc, Nt = 20, 4
    dt = 8.0 * (2.0 / nc) / (40 / np.pi)              # CFL = |w| dt / h ~ 8 at the boundary of the rotating field
    omesh = SquareMesh(-1, 1, nc)
    asm = P1Assembler(omesh)
    n = omesh.nodes
    rng = np.random.default_rng(8)
    u0 = np.exp(-20 * ((omesh.x + 0.3) ** 2 + (omesh.y - 0.2) ** 2))[omesh.dof_to_vertex]
    ck = 0.5 * rng.random((Nt + 1) * n)
    sb = otraj.SolidBody(asm, om=np.pi / 40)
    uo = np.zeros((Nt + 1) * n); uo[:n] = u0
    otraj.solidbody_forward(sb, ck, uo, n, Nt, dt)
    po = otraj.solidbody_adjoint(sb, ck, uo, 0.9 * uo[Nt * n:], np.zeros_like(uo), n, Nt, dt)
    prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, nc), Nt, dt)
    try:
        ug = np.zeros((Nt + 1) * n); ug[:n] = u0
        prob.solve_state(ck, ug)
        log = prob.solver_log(1)
        assert np.all(log["flags"] & hp.FLAG_MMATRIX_ROWSUM)
        assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET) and log["solver_resid"].max() <= 1e-13
        assert np.linalg.norm(ug - uo) / np.linalg.norm(uo) < 1e-9
        pg = prob.solve_adjoint(ck, ug, 0.9 * uo[Nt * n:], np.zeros_like(ug))
        assert np.linalg.norm(pg - po) / np.linalg.norm(po) < 1e-9
        # the choice is remembered per kind of sweep: a second forward sweep goes straight to BiCGStab and agrees
        ug2 = np.zeros((Nt + 1) * n); ug2[:n] = u0
        prob.solve_state(ck, ug2)
        assert np.array_equal(ug2, ug)
    finally:
        prob.close()
