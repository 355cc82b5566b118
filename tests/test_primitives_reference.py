"""tests/primitives_reference.py against the oracle (oracle.fct, oracle.traj) and the reference's own outputs
(tests/golden/kernels.npz), with the tolerances tests/test_oracle_golden.py::test_small_kernels holds those quantities
to -- the helper is pinned here before tests/test_gpu_primitives.py measures the device against it.  No GPU."""
import numpy as np
import pytest

import primitives_reference as pr
from helpers_golden import load, csr_from
from oracle import fct as ofct
from oracle import traj as otraj
from oracle.assembly import P1Assembler, row_lump_diag
from oracle.mesh import SquareMesh


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def csr_of(A):
    A = A.tocsr().copy()
    A.sort_indices()
    return A.indptr, A.indices, A.data


@pytest.fixture(scope="module")
def golden():
    z = load("kernels.npz")
    a1, a2, nc = z["geom"]
    mesh = SquareMesh(a1, a2, int(nc))
    asm = P1Assembler(mesh)
    return z, mesh, asm, asm.mass()


def test_chebsi_vs_oracle_and_reference(golden):
    z, mesh, asm, M = golden
    csr = csr_of(M)
    it = pr.chebsi_iterates(*csr, M.diagonal(), z["cheb_b"], [1, 2, 3, 7, 20])
    assert rel(it[20], z["cheb_y"]) < 1e-14                       # the reference's own ChebSI output
    for k, y in it.items():                                       # one recurrence serves every count
        assert rel(y, ofct.chebsi(z["cheb_b"], M, M.diagonal(), k, 0.5, 2)) < 1e-14, k
    md = M.diagonal() * (1 + 0.3 * np.random.default_rng(0).random(M.shape[0]))
    for k, y in pr.chebsi_iterates(*csr, md, z["cheb_b"], [1, 12], 0.25, 3.0).items():
        assert rel(y, ofct.chebsi(z["cheb_b"], M, md, k, 0.25, 3.0)) < 1e-14, k


def test_matvec_and_spmv(golden):
    z, mesh, asm, M = golden
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(M.shape[0]), rng.standard_normal(M.shape[0])
    val, scale = pr.spmv(*csr_of(M), x, -2.5, 0.5, y)
    assert np.all(np.abs(val - (-2.5 * (M @ x) + 0.5 * y)) <= 9 * pr.U * scale)
    val0, _ = pr.spmv(*csr_of(M), x, 1.0, 0.0, np.full_like(y, np.nan))
    assert np.all(np.isfinite(val0)) and rel(val0, M @ x) < 1e-15


def test_artificial_diffusion_and_transpose(golden):
    z, mesh, asm, M = golden
    n = mesh.nodes
    pat = ofct.Pattern(M)
    K = csr_from(z, "K", n)
    ip, ix = pat.indptr, pat.indices
    k = pat.values(K)
    d = pr.artificial_diffusion_offdiag(ip, ix, k)
    od = ofct.artificial_diffusion(pat, k)
    assert np.array_equal(d[pat.offd], od[pat.offd])              # max(0, -k_ij, -k_ji): exact either way
    assert np.max(np.abs(d - pat.values(csr_from(z, "D", n)))[pat.offd]) < 1e-15      # the reference's own D
    assert np.array_equal(np.add.reduceat(d, ip[:-1]), -od[pat.diag_pos])
    assert np.array_equal(pr.transpose_values(ip, ix, k), pat.values(pat.csr(k).T.tocsr()))
    # ELL layout: slot 0 the diagonal, a slot whose column is the row itself is padding and holds 0
    A = pat.csr(np.arange(1.0, pat.nnz + 1))
    cols = np.stack([np.arange(n), np.minimum(np.arange(n) + 1, n - 1)]).astype(np.int32)
    ell = pr.ell_layout(cols, *csr_of(A))
    assert np.array_equal(ell[0], A.diagonal()) and ell[1, n - 1] == 0.0
    assert np.array_equal(ell[1, :n - 1], np.asarray(A[np.arange(n - 1), np.arange(1, n)]).ravel())


def test_reductions_vs_oracle_and_reference(golden):
    z, mesh, asm, M = golden
    n = mesh.nodes
    csr = csr_of(M)
    Nt, dt, beta = int(z["Nt"]), float(z["dt"]), float(z["beta"])

    def close(got, ref):
        return abs(float(got[0]) - ref) < 1e-13 * abs(ref) and float(got[1]) >= abs(ref)

    assert close(pr.norm_sq_Q(csr, z["phi"], None, Nt, dt), z["L2Q"])
    assert close(pr.norm_sq_Q(csr, z["phi"], None, Nt, dt), ofct.l2_norm_sq_Q(z["phi"], Nt, dt, M))
    assert close(pr.norm_sq_Q(csr, z["phi"], z["tgt"], Nt, dt), ofct.l2_norm_sq_Q(z["phi"] - z["tgt"], Nt, dt, M))
    assert close(pr.norm_sq_Omega(csr, z["phi"][:n], None), z["L2Omega"])
    assert close(pr.norm_sq_Omega(csr, z["phi"][:n], z["tgt"][:n]), ofct.l2_norm_sq_Omega((z["phi"] - z["tgt"])[:n], M))
    assert close(pr.cost(csr, z["phi"], z["tgt"], z["ctl"], Nt, dt, beta, "alltime"), z["J_alltime_1"])
    assert close(pr.cost(csr, z["phi"], z["tgt"], z["ctl"], Nt, dt, beta, "alltime", z["phi2"], z["tgt2"]), z["J_alltime_2"])
    assert close(pr.cost(csr, z["phi"], z["tgt"][:n], z["ctl"], Nt, dt, beta, "finaltime"), z["J_finaltime_1"])
    assert close(pr.cost(csr, z["phi"], z["tgt"][:n], z["ctl"], Nt, dt, beta, "finaltime", z["phi2"], z["tgt2"][:n]),
                 z["J_finaltime_2"])
    J = ofct.cost_functional(z["phi"], z["tgt"][:n], z["ctl"], Nt, dt, M, beta, "finaltime", var2=z["phi2"],
                             var2_target=z["tgt2"][:n])
    assert close(pr.cost(csr, z["phi"], z["tgt"][:n], z["ctl"], Nt, dt, beta, "finaltime", z["phi2"], z["tgt2"][:n]), J)
    one = pr.norm_sq_Q(csr, z["phi"][:2 * n], None, 1, dt)        # num_steps = 1: two half-weight levels
    assert close(one, ofct.l2_norm_sq_Q(z["phi"][:2 * n], 1, dt, M))


@pytest.mark.parametrize("drift", [(1.0, 1.0), (0.7, -1.3)])
def test_drift_rhs_vs_oracle(drift):
    """The pre-Chebyshev vector of oracle.traj.solidbody_descent_direction, in both node numberings, and the closed form
    for u linear in x, p = 1: int p (b.grad u) v = bx * ml_i."""
    nc, Nt, beta = 12, 2, 0.1
    mesh = SquareMesh(0.0, 1.0, nc)
    asm = P1Assembler(mesh)
    n = mesh.nodes
    sb = otraj.SolidBody(asm, om=1.0, drift=drift)
    M = asm.mass()
    rng = np.random.default_rng(3)
    ck, uk, pk = (rng.standard_normal((Nt + 1) * n) for _ in range(3))
    v2d = mesh.vertex_to_dof
    Mv = M[v2d][:, v2d]                                             # the same matrix in vertex numbering
    geom = pr.p1_geometry(mesh)
    # the assembler's float64 geometry against the same formulas in longdouble: the cancellation of its coordinate
    # differences, (n_cells + 1) u per edge, two edges in the determinant and a few operations more
    tol = 4 * (nc + 1) * pr.U
    assert np.all(np.abs(geom[1] - asm.MK) <= tol * np.abs(geom[1]))
    assert np.all(np.abs(geom[0] - asm.grad) <= tol * np.abs(geom[0]).max())
    for lvl in range(Nt + 1):
        o = otraj.solidbody_descent_rhs(sb, ck, uk, pk, beta, n, lvl)
        sl = slice(lvl * n, (lvl + 1) * n)
        val, sabs = pr.drift_rhs(geom, asm.dof, *csr_of(M), ck[sl], uk[sl], pk[sl], beta, drift)
        # the oracle's own float64 chain (twice the 16 operations the device is held to) on its float64 geometry (tol, in
        # the gradient and in the element mass matrix)
        assert np.all(np.abs(val - o) <= (32 * pr.U + 2 * tol) * sabs)
        valv, sabsv = pr.drift_rhs(geom, mesh.cells, *csr_of(Mv), ck[sl][v2d], uk[sl][v2d], pk[sl][v2d], beta, drift)
        assert np.array_equal(valv, val[v2d]) or np.all(np.abs(valv - val[v2d]) <= 2 * pr.U * sabsv)
    x_dof = mesh.x[mesh.dof_to_vertex]
    val, sabs = pr.drift_rhs(geom, asm.dof, *csr_of(M), np.zeros(n), x_dof, np.ones(n), 0.0, drift)
    ml = pr.lumped_mass(geom, asm.dof, n)
    assert np.all(np.abs(ml.astype(np.float64) - row_lump_diag(M)) <= tol * row_lump_diag(M))
    # x_dof = fl(a1 + i h) carries u |x| <= u per node, 1 / h of it in the gradient: (n_cells + 2) u of the terms
    assert np.all(np.abs(val + (drift[0] * ml).astype(np.float64)) <= (nc + 2) * pr.U * sabs)


def test_descent_direction_unchanged_by_the_refactor():
    """solidbody_descent_direction == ChebSI of solidbody_descent_rhs, level by level (bitwise)."""
    mesh = SquareMesh(-1.0, 1.0, 6)
    asm = P1Assembler(mesh)
    n, Nt = mesh.nodes, 2
    sb = otraj.SolidBody(asm, om=2.0)
    rng = np.random.default_rng(4)
    ck, uk, pk = (rng.random((Nt + 1) * n) for _ in range(3))
    dk = otraj.solidbody_descent_direction(sb, ck, uk, pk, 0.05, n, Nt)
    M = sb.cm.M
    for lvl in range(Nt + 1):
        rhs = otraj.solidbody_descent_rhs(sb, ck, uk, pk, 0.05, n, lvl)
        assert np.array_equal(dk[lvl * n:(lvl + 1) * n], ofct.chebsi(rhs, M, M.diagonal(), 20, 0.5, 2))


def test_elementwise_expressions():
    rng = np.random.default_rng(5)
    c, d, g = rng.standard_normal(300), rng.standard_normal(300), rng.standard_normal(300)
    out = pr.clip_axpy(c, 0.5, d, -0.4, 0.6)
    assert np.array_equal(out, np.clip(c + 0.5 * d, -0.4, 0.6)) and out.min() == -0.4 and out.max() == 0.6
    assert np.array_equal(pr.axpby(2.0, c, -3.0, d), 2.0 * c + -3.0 * d) and np.array_equal(pr.axpby(2.0, c, 1.0, None), 2.0 * c)
    co, so = pr.source_trials(c, d, g, 0.8, 3, -0.4, 0.6)
    assert np.array_equal(co[2], np.clip(c + 0.2 * d, -0.4, 0.6)) and np.array_equal(so[1], g + co[1])
    assert np.array_equal(pr.source_trials(c, d, None, 0.8, 1, -0.4, 0.6)[1][0], co[0])
    assert np.array_equal(pr.descent_pointwise(0.1, c, d, y=g, divisor=0.3), -(0.1 * c - d * g / 0.3))
    assert np.array_equal(pr.descent_pointwise(0.1, c, d, scale=7.0), -(0.1 * c - 7.0 * d))
