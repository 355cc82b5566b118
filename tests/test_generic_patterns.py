"""CPU preconditions of the GPU tests on general sparsity patterns (tests/generic_patterns.py): the patterns are what their
names say, the data makes the low-order solve converge and the limiter cut, and it has the power to tell a subtly wrong
scheme from the right one."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import generic_patterns as gp
from oracle import fct as ofct

EDGED = tuple(k for k in gp.NAMES if k not in gp.NO_EDGE)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_STEPS = {}


def oracle_step(name):
    """(u, info) of oracle.fct.fct_step on member 0 of problem(name), computed once"""
    if name not in _STEPS:
        P = gp.problem(name, 1)
        info = {}
        u = ofct.fct_step(P.A[0], P.rhs[0], P.u_n[0], P.dt, P.n, P.M, P.ML, None, non_flux_mat=P.N, info=info)
        _STEPS[name] = (np.atleast_1d(u), info)
    return _STEPS[name]


@pytest.mark.parametrize("name", list(gp.GENERATORS))
def test_pattern_is_what_its_name_states(name):
    M, A = gp.matrices(name)
    assert M.shape == A.shape == (gp.NODES[name], gp.NODES[name])
    assert M.has_sorted_indices and np.array_equal(M.indptr, A.indptr) and np.array_equal(M.indices, A.indices)
    ofct.Pattern(M)                                                      # structurally symmetric, full diagonal (raises)
    assert np.all(M.diagonal() > 0) and gp.width(M) == gp.WIDTH[name]
    assert (gp.WIDTH[name] > gp.MAX_W) == (name in gp.REFUSED)
    assert abs(M - M.T).max() == 0.0
    off = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)) != M.indices
    assert np.all(M.data[off] > 0)


def test_shapes_the_names_promise():
    lens = lambda name: np.diff(gp.matrices(name)[0].indptr)
    assert sorted(lens("star15").tolist()) == [2] * 15 + [16]
    l = lens("hub300")
    assert l[150] == 16 and np.all(np.delete(l, 150) <= 4) and (l == 3).sum() > 280
    assert gp.bandwidth(gp.matrices("hub300")[0]) == 149
    assert gp.bandwidth(gp.matrices("band7a")[0]) == 5 and gp.bandwidth(gp.matrices("band7b")[0]) == 38
    for name, strips in (("band7a", 3), ("band7b", 4)):                   # several strips, hence seams
        assert -(-gp.NODES[name] // gp.STRIP_ROWS[name]) == strips
    assert (lens("grid3d7") == 15).sum() == 5 ** 3 and lens("grid3d7").max() == 15     # the interior nodes
    l = lens("delaunay700")
    assert l.min() == 4 and l.max() == 12                                 # degrees + 1
    assert gp.bandwidth(gp.matrices("delaunay700")[0]) > 600
    assert gp.bandwidth(gp.matrices("delaunay700_rcm")[0]) < 120
    assert gp.bandwidth(gp.matrices("mesh26_perm")[0]) > 600
    assert np.array_equal(np.sort(lens("delaunay700")), np.sort(lens("delaunay700_rcm")))


@pytest.mark.parametrize("name", gp.NAMES)
def test_synthetic_data_is_as_described(name):
    M, A = gp.matrices(name)
    P = gp.problem(name, 3)
    rows = np.repeat(np.arange(P.n), np.diff(M.indptr))
    off = rows != M.indices
    if name not in gp.P1_NAMES:
        offsum = np.add.reduceat(np.where(off, M.data, 0.0), M.indptr[:-1])
        assert np.allclose(M.diagonal(), 2 * offsum + 1, rtol=1e-15, atol=0)
        if off.sum() >= 100:
            zeros = (A.data[off] == 0).mean()
            assert 0.2 < zeros < 0.4 and (A.data[off] > 0).any() and (A.data[off] < 0).any()
    # the spectrum of diag(M)^-1 M inside ChebSI's [0.5, 2]
    ev = np.linalg.eigvals(M.toarray() / M.diagonal()[:, None]).real if P.n <= 700 else None
    if ev is not None:
        assert ev.min() >= 0.5 - 1e-12 and ev.max() <= 2.0 + 1e-12
    for m in range(3):
        assert np.all(P.u_n[m][:P.n // 3] == P.u_n[m][0]) and np.array_equal(P.A[m].indices, M.indices)
        if m and off.any():
            assert not np.array_equal(P.A[m].data, P.A[0].data)
    assert abs(P.N - 0.05 * M).max() < 1e-17


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", gp.NAMES)
def test_jacobi_norm(name, B):
    P = gp.problem(name, B)
    assert 0 < P.dt <= 1.0
    for m in range(B):
        for Nmat in (None, P.N):
            g = gp.jacobi_norm(P.M, P.A[m], P.ml, P.dt, Nmat)
            diag, _ = gp.low_order(P.M, P.A[m], P.ml, P.dt, Nmat)
            assert np.all(diag > 0) and g <= 0.5, (name, m, g)
    if B == 1 and P.dt < 1.0:                                             # dt is half of the largest admissible one
        assert abs(gp.jacobi_norm(P.M, P.A[0], P.ml, 2 * P.dt) - 0.5) < 1e-12


@pytest.mark.parametrize("name", gp.NAMES)
def test_limiter_cuts_and_output_is_finite(name):
    u, info = oracle_step(name)
    assert u.shape == (gp.NODES[name],) and np.all(np.isfinite(u))
    cut = np.mean((info["r_pos"] < 1) | (info["r_neg"] < 1))
    print(f"[generic] {name}: dt={gp.problem(name).dt:.4f} jacobi={gp.jacobi_norm(*_args(name)):.3f} cut rows={cut:.2f}")
    if name in gp.NO_EDGE:
        assert cut == 0.0
    else:
        assert cut >= 0.25, cut


def _args(name):
    P = gp.problem(name, 1)
    return P.M, P.A[0], P.ml, P.dt, P.N


def test_restated_step_is_the_oracles():
    for name in gp.NAMES:
        P = gp.problem(name, 1)
        u = gp.spoilt_step(P.A[0], P.rhs[0], P.u_n[0], P.dt, P.M, P.ml, P.N, spoil=None)
        assert rel(u, oracle_step(name)[0]) < 1e-14, name


def test_data_tells_a_spoilt_scheme_from_the_true_one():
    """Every pattern with an edge tells at least one spoilt rule from the true step by more than 1e-6 relative l2, and
    every spoilt rule is told on at least three patterns."""
    told = {s: [] for s in gp.SPOILS}
    for name in EDGED:
        P = gp.problem(name, 1)
        ref = oracle_step(name)[0]
        errs = {s: rel(gp.spoilt_step(P.A[0], P.rhs[0], P.u_n[0], P.dt, P.M, P.ml, P.N, spoil=s), ref) for s in gp.SPOILS}
        print(f"[generic] power {name}: " + ", ".join(f"{s}={e:.2e}" for s, e in errs.items()))
        assert max(errs.values()) > 1e-6, (name, errs)
        for s, e in errs.items():
            if e > 1e-6:
                told[s].append(name)
    for s in gp.SPOILS:
        assert len(told[s]) >= 3, (s, told[s])


def test_conservative_operator_has_zero_column_sums():
    for name in ("hub300", "delaunay700"):
        A = gp.conservative(gp.problem(name).A[0])
        assert np.array_equal(A.indices, gp.matrices(name)[0].indices)
        assert np.abs(np.asarray(A.sum(axis=0))).max() < 1e-13 * max(np.abs(A.data).max(), 1.0)


def test_mesh26_perm_is_the_square_mesh_renumbered():
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    mesh = SquareMesh(0.0, 1.0, gp.MESH26_CELLS)
    v2d = mesh.vertex_to_dof
    Mo = csr_matrix(P1Assembler(mesh).mass()[v2d][:, v2d])
    Mv, _ = gp.mesh26_vertex_order()
    assert abs(Mo - Mv).max() < 1e-15 * Mv.diagonal().max() * 64
    perm = gp.mesh26_perm()
    Mp, Ap = gp.matrices("mesh26_perm")
    _, Av = gp.mesh26_vertex_order()
    assert abs(Mp[perm][:, perm] - Mv).max() == 0.0 and abs(Ap[perm][:, perm] - Av).max() == 0.0
