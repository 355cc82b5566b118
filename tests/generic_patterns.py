"""Sparsity patterns that are not the structured square mesh, with data that makes an FCT step on them worth checking
(a helper, not a test; NumPy / SciPy only).  tests/test_generic_patterns.py pins the properties claimed here on the CPU,
tests/test_gpu_generic_patterns.py and tests/test_gpu_primitives.py run the device on them.

Every generator returns (M, A): sorted CSR matrices on ONE structurally symmetric pattern with a full diagonal (A keeps
its exact zeros as stored entries).
  synthetic   M symmetric, off-diagonals in [0.25, 0.75], diagonal = 2 * (off-diagonal row sum) + 1, so the spectrum of
              diag(M)^-1 M lies in 1 -+ 1/2 (Gershgorin), inside ChebSI's default [0.5, 2];
              A mixed sign, about 30 % exact zeros off the diagonal, not symmetric.
  P1          M the P1 mass matrix of a triangulation (spectrum of diag(M)^-1 M in [0.5, 2]),
              A = convection of the rotation wind (-y, x) about the centre + 1e-3 * stiffness.

problem(name, B) adds the other inputs of a step, see there.  spoilt_step restates the oracle's step with one rule of the
scheme broken at a time: the CPU test shows that the data tells each of them from the true step.
"""
from dataclasses import dataclass, field

import numpy as np
from scipy.sparse import coo_matrix, csr_matrix, diags
from scipy.sparse.linalg import spsolve

MAX_W = 16           # FEMFCT_MAX_W of csrc/femfct_internal.h: entries per row, the diagonal included


# ------------------------------------------------------------------------------------------------ patterns
def _pattern(n, edges):
    """(indptr, indices) of the graph's adjacency plus the diagonal, sorted columns"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    i = np.concatenate([e[:, 0], e[:, 1], np.arange(n)])
    j = np.concatenate([e[:, 1], e[:, 0], np.arange(n)])
    P = coo_matrix((np.ones(i.size), (i, j)), shape=(n, n)).tocsr()
    P.sum_duplicates()
    P.sort_indices()
    return P.indptr.astype(np.int32), P.indices.astype(np.int32)


def _rows(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


def _synthetic(n, edges, seed):
    indptr, indices = _pattern(n, edges)
    rows, cols = _rows(indptr), indices.astype(np.int64)
    rng = np.random.default_rng(seed)
    off = rows != cols
    # one value per undirected edge: drawn for the stored entries of the upper triangle, mirrored by the edge's key
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = lo * n + hi
    uniq, inv = np.unique(key[off], return_inverse=True)
    m = np.zeros(rows.size)
    m[off] = (0.25 + 0.5 * rng.random(uniq.size))[inv]
    m[~off] = 2.0 * np.add.reduceat(m, indptr[:-1]) + 1.0
    a = rng.standard_normal(rows.size)
    a[off & (rng.random(rows.size) < 0.3)] = 0.0
    a[~off] *= 0.3
    return (csr_matrix((m, indices, indptr), shape=(n, n)), csr_matrix((a, indices, indptr), shape=(n, n)))


def _p1(x, y, cells):
    """P1 mass matrix and convection of the wind (-(y - yc), x - xc) + 1e-3 stiffness on the triangles `cells`; the wind is
    linear, so its element integral int_K w phi_i = |K| / 12 (w_0 + w_1 + w_2 + w_i) is exact"""
    n = x.size
    c = np.asarray(cells, dtype=np.int64)
    X, Y = x[c], y[c]
    e1x, e1y, e2x, e2y = X[:, 1] - X[:, 0], Y[:, 1] - Y[:, 0], X[:, 2] - X[:, 0], Y[:, 2] - Y[:, 0]
    det = e1x * e2y - e1y * e2x
    area = np.abs(det) / 2
    g = np.empty((c.shape[0], 3, 2))
    g[:, 1, 0], g[:, 1, 1] = e2y / det, -e2x / det
    g[:, 2, 0], g[:, 2, 1] = -e1y / det, e1x / det
    g[:, 0] = -(g[:, 1] + g[:, 2])
    xc, yc = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
    w = np.stack([-(Y - yc), X - xc], axis=2)                                        # (nt, 3, 2) wind at the vertices
    wi = (area[:, None, None] / 12) * (w.sum(axis=1)[:, None, :] + w)               # int_K w phi_i
    Me = (area[:, None, None] / 12) * (np.ones((3, 3)) + np.eye(3))[None]
    Se = area[:, None, None] * np.einsum("tid,tjd->tij", g, g)
    Ce = np.einsum("tid,tjd->tij", wi, g)                                            # int (w . grad phi_j) phi_i
    i, j = np.repeat(c, 3, axis=1).ravel(), np.tile(c, (1, 3)).ravel()

    def mat(Ke):
        K = coo_matrix((Ke.ravel(), (i, j)), shape=(n, n)).tocsr()
        K.sum_duplicates()
        K.sort_indices()
        return K

    M, S, C = mat(Me), mat(Se), mat(Ce)
    assert np.array_equal(M.indices, S.indices) and np.array_equal(M.indices, C.indices)
    A = csr_matrix((C.data + 1e-3 * S.data, M.indices, M.indptr), shape=(n, n))
    return M, A


def _permuted(M, A, perm):
    """the matrices in the numbering new = perm[old]"""
    out = []
    for K in (M, A):
        Kc = K.tocoo()
        P = coo_matrix((Kc.data, (perm[Kc.row], perm[Kc.col])), shape=K.shape).tocsr()   # stored zeros stay stored
        P.sort_indices()
        out.append(P)
    assert np.array_equal(out[0].indices, out[1].indices) and np.array_equal(out[0].indptr, out[1].indptr)
    return out[0], out[1]


def _offsets_1d(n, offs):
    return [(i, i + o) for o in offs for i in range(n - o)]


def _single():
    return _synthetic(1, [], 1)


def _diag5():
    return _synthetic(5, [], 5)


def _pair():
    return _synthetic(2, [(0, 1)], 2)


def _path67():
    return _synthetic(67, _offsets_1d(67, (1,)), 67)


def _star(leaves, seed):
    return _synthetic(leaves + 1, [(0, k) for k in range(1, leaves + 1)], seed)


HUB300_FAR = (3, 17, 40, 66, 95, 120, 180, 205, 231, 250, 270, 288, 299)


def _hub300():
    return _synthetic(300, _offsets_1d(300, (1,)) + [(150, k) for k in HUB300_FAR], 300)


def _grid3d7():
    N = 7
    idx = np.arange(N ** 3).reshape(N, N, N)
    edges = []
    for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
        a = idx[:N - d[0], :N - d[1], :N - d[2]].ravel()
        b = idx[d[0]:, d[1]:, d[2]:].ravel()
        edges += list(zip(a.tolist(), b.tolist()))
    return _synthetic(N ** 3, edges, 343)


def _band7a():
    return _synthetic(4500, _offsets_1d(4500, (1, 2, 5)), 4501)


def _band7b():
    return _synthetic(4500, _offsets_1d(4500, (1, 37, 38)), 4502)


def _delaunay700():
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(701).random((700, 2))
    return _p1(pts[:, 0].copy(), pts[:, 1].copy(), Delaunay(pts).simplices)


def _delaunay700_rcm():
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    M, A = _delaunay700()
    order = np.asarray(reverse_cuthill_mckee(M, symmetric_mode=True), dtype=np.int64)    # order[new] = old
    perm = np.empty_like(order)
    perm[order] = np.arange(order.size)
    return _permuted(M, A, perm)


MESH26_CELLS = 25


def mesh26_perm():
    """perm[v] = the node that vertex v (natural order, iy * 26 + ix) of the 26 x 26 unit-square mesh becomes"""
    return np.random.default_rng(26).permutation((MESH26_CELLS + 1) ** 2)


def square_mesh_matrices(n_cells, fenics=False):
    """the P1 matrices of the structured mesh of the unit square in the natural vertex order, or in the FEniCS order"""
    from oracle.mesh import SquareMesh
    mesh = SquareMesh(0.0, 1.0, n_cells)
    M, A = _p1(mesh.x, mesh.y, mesh.cells)
    return _permuted(M, A, np.asarray(mesh.vertex_to_dof, dtype=np.int64)) if fenics else (M, A)


def mesh26_vertex_order():
    return square_mesh_matrices(MESH26_CELLS)


def _mesh26_perm():
    M, A = mesh26_vertex_order()
    return _permuted(M, A, mesh26_perm())


GENERATORS = {
    "single": _single, "diag5": _diag5, "pair": _pair, "path67": _path67, "star15": lambda: _star(15, 15),
    "hub300": _hub300, "grid3d7": _grid3d7, "band7a": _band7a, "band7b": _band7b, "delaunay700": _delaunay700,
    "delaunay700_rcm": _delaunay700_rcm, "mesh26_perm": _mesh26_perm, "star16": lambda: _star(16, 16),
}
REFUSED = ("star16",)                                    # a row of 17 entries
NAMES = tuple(k for k in GENERATORS if k not in REFUSED)
NO_EDGE = ("single", "diag5")
P1_NAMES = ("delaunay700", "delaunay700_rcm", "mesh26_perm")
# ELL width (longest row, diagonal included) and number of nodes each name stands for; the Delaunay triangulation's comes
# from its seed (vertex degrees 3 .. 11)
WIDTH = {"single": 1, "diag5": 1, "pair": 2, "path67": 3, "star15": 16, "hub300": 16, "grid3d7": 15, "band7a": 7,
         "band7b": 7, "delaunay700": 12, "delaunay700_rcm": 12, "mesh26_perm": 7, "star16": 17}
NODES = {"single": 1, "diag5": 5, "pair": 2, "path67": 67, "star15": 16, "hub300": 300, "grid3d7": 343, "band7a": 4500,
         "band7b": 4500, "delaunay700": 700, "delaunay700_rcm": 700, "mesh26_perm": 676, "star16": 17}
# rows owned by a workgroup of the row-strip kernels (femfct_strip_plan: K = 8 sweeps, halo 8 * bandwidth, two rows per
# thread of 1024: R = 2048 - 16 * bandwidth), hence 3 and 4 strips of the 4500 rows
STRIP_ROWS = {"band7a": 2048 - 16 * 5, "band7b": 2048 - 16 * 38}

_CACHE = {}


def matrices(name):
    if name not in _CACHE:
        M, A = GENERATORS[name]()
        _CACHE[name] = (M, A)
    return _CACHE[name]


def bandwidth(M):
    M = csr_matrix(M)
    return int(np.max(np.abs(_rows(M.indptr) - M.indices))) if M.nnz else 0


def width(M):
    return int(np.diff(csr_matrix(M).indptr).max())


# ------------------------------------------------------------------------------------------------ a step's inputs
def offdiag_transposed(M, vals):
    """values of the transposed entries, on M's (symmetric) pattern"""
    T = csr_matrix((vals, M.indices, M.indptr), shape=M.shape).T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, M.indices)
    return T.data


def low_order(M, A, ml, dt, Nmat=None):
    """(diagonal, sum of |off-diagonals| per row) of L = ML + dt (A - D) (+ dt N), D from max(0, a_ij, a_ji)"""
    rows, off = _rows(M.indptr), _rows(M.indptr) != M.indices
    a = A.data
    d = np.where(off, np.maximum(0.0, np.maximum(a, offdiag_transposed(M, a))), 0.0)
    dsum = np.add.reduceat(d, M.indptr[:-1])
    l = a - d
    if Nmat is not None:
        l = l + Nmat.data
    s = np.add.reduceat(np.where(off, np.abs(l), 0.0), M.indptr[:-1])
    c = l[~off] + dsum                                            # a_ii - d_ii, d_ii = -sum_j d_ij
    return ml + dt * c, dt * s


def jacobi_norm(M, A, ml, dt, Nmat=None):
    """infinity norm of the Jacobi iteration matrix of L"""
    diag, s = low_order(M, A, ml, dt, Nmat)
    return float(np.max(s / np.abs(diag)))


def time_step(M, A, ml):
    """half the largest dt for which the Jacobi iteration matrix of L = ML + dt (A - D) has infinity norm <= 1/2, at most 1.
    Row i: dt s_i <= (ml_i + dt c_i) / 2 with s_i the absolute off-diagonal sum of A - D and c_i = a_ii - d_ii, i.e.
    dt (s_i - c_i / 2) <= ml_i / 2, a bound only where s_i > c_i / 2 (and then it also keeps ml_i + dt c_i > 0)."""
    diag1, s1 = low_order(M, A, np.zeros(M.shape[0]), 1.0)        # c_i and s_i
    den = s1 - 0.5 * diag1
    bound = np.full(M.shape[0], np.inf)
    bound[den > 0] = 0.5 * ml[den > 0] / den[den > 0]
    return float(min(1.0, 0.5 * bound.min()))


@dataclass
class Problem:
    name: str
    M: csr_matrix
    ml: np.ndarray
    ML: csr_matrix
    N: csr_matrix
    dt: float
    A: list = field(default_factory=list)            # per member
    u_n: list = field(default_factory=list)
    rhs: list = field(default_factory=list)

    @property
    def n(self):
        return self.M.shape[0]


def member_matrix(name, m):
    """member 0 has the generator's A; the others its entries redrawn (synthetic) or rescaled (P1)"""
    M, A = matrices(name)
    if m == 0:
        return A
    if name in P1_NAMES:
        return rescaled(A, m)
    rng = np.random.default_rng(1000 * m + M.shape[0])
    off = _rows(M.indptr) != M.indices
    a = rng.standard_normal(A.nnz)
    a[off & (rng.random(A.nnz) < 0.3)] = 0.0
    a[~off] *= 0.3
    return csr_matrix((a, A.indices, A.indptr), shape=A.shape)


_PROBLEMS = {}


def problem(name, B=1):
    """The inputs of a step with B members on one pattern: own A, u_n (random, the first third of the nodes on an exact
    plateau) and rhs per member, N = 0.05 M, and one dt: the smallest of the members' time_step."""
    if (name, B) not in _PROBLEMS:
        _PROBLEMS[(name, B)] = problem_of(name, matrices(name)[0], [member_matrix(name, m) for m in range(B)])
    return _PROBLEMS[(name, B)]


def problem_of(name, M, As):
    """the same for a mass matrix and the members' flux matrices as given (lumped mass: the row sums of M)"""
    n = M.shape[0]
    ml = np.asarray(M.sum(axis=1)).ravel()
    P = Problem(name, M, ml, diags(ml).tocsr(), csr_matrix((0.05 * M.data, M.indices, M.indptr), shape=M.shape), 1.0)
    for m, A in enumerate(As):
        rng = np.random.default_rng(7 * n + m)
        u = rng.random(n)
        u[:n // 3] = 0.5 + 0.125 * m
        P.A.append(A)
        P.u_n.append(u)
        P.rhs.append(0.1 * rng.standard_normal(n))
        P.dt = min(P.dt, time_step(M, A, ml))
    return P


def rescaled(A, m):
    """a member's own flux matrix: A's entries scaled by factors in [0.5, 1.5] (member 0: A itself)"""
    if m == 0:
        return A
    rng = np.random.default_rng(1000 * m + A.shape[0])
    return csr_matrix((A.data * (0.5 + rng.random(A.nnz)), A.indices, A.indptr), shape=A.shape)


def conservative(A):
    """A_c = A - diag(column sums of A): its columns sum to zero, so a step with rhs = 0 and no N conserves sum ml_i u_i"""
    A = csr_matrix(A)
    colsum = np.asarray(A.sum(axis=0)).ravel()
    data = A.data.copy()
    diag = _rows(A.indptr) == A.indices
    data[diag] -= colsum
    return csr_matrix((data, A.indices, A.indptr), shape=A.shape)


# ------------------------------------------------------------------------------------------------ the power check
SPOILS = ("d_one_sided", "r_swapped", "q_without_self")


def spoilt_step(A, rhs, u_n, dt, M, ml, Nmat=None, spoil=None):
    """The FEM-FCT step of oracle.fct.fct_step, restated, with one rule broken:
         d_one_sided      d_ij = max(0, a_ij), the transposed entry left out;
         r_swapped        r_pos and r_neg exchanged in the choice of alpha_ij;
         q_without_self   the local extrema of u_low taken over the neighbours without the row itself.
    spoil=None is the true step (pinned against the oracle by the CPU test)."""
    from oracle.fct import chebsi
    M = csr_matrix(M)
    n = M.shape[0]
    indptr, cols = M.indptr, M.indices.astype(np.int64)
    rows = _rows(indptr)
    off = rows != cols
    a, m = A.data, M.data
    at = offdiag_transposed(M, a)
    if spoil == "d_one_sided":
        d = np.where(off, np.maximum(0.0, a), 0.0)
    else:
        d = np.where(off, np.maximum(0.0, np.maximum(a, at)), 0.0)
    d[~off] = -np.add.reduceat(d, indptr[:-1])
    l = dt * (a - d)
    l[~off] += ml
    if Nmat is not None:
        l = l + dt * Nmat.data
    mk = lambda v: csr_matrix((v, M.indices, indptr), shape=(n, n))
    u_low = np.atleast_1d(spsolve(mk(l).tocsc(), ml * u_n + dt * rhs))
    du = chebsi(-(mk(a) @ u_low) + rhs, M, m[~off], 20, 0.5, 2)
    f = np.where(off, m * (du[rows] - du[cols]) + d * (u_low[rows] - u_low[cols]), 0.0)
    p_pos = np.add.reduceat(np.maximum(f, 0.0), indptr[:-1])
    p_neg = np.add.reduceat(np.minimum(f, 0.0), indptr[:-1])
    nb = u_low[cols]
    if spoil == "q_without_self":
        q_pos = np.maximum.reduceat(np.where(off, nb, -np.inf), indptr[:-1]) - u_low
        q_neg = np.minimum.reduceat(np.where(off, nb, np.inf), indptr[:-1]) - u_low
    else:
        q_pos = np.maximum.reduceat(nb, indptr[:-1]) - u_low
        q_neg = np.minimum.reduceat(nb, indptr[:-1]) - u_low
    r_pos, r_neg = np.ones(n), np.ones(n)
    kp, kn = p_pos != 0, p_neg != 0
    r_pos[kp] = np.minimum(1, ml[kp] * q_pos[kp] / (dt * p_pos[kp]))
    r_neg[kn] = np.minimum(1, ml[kn] * q_neg[kn] / (dt * p_neg[kn]))
    if spoil == "r_swapped":
        alpha = np.where(f > 0, np.minimum(r_neg[rows], r_pos[cols]), np.minimum(r_pos[rows], r_neg[cols]))
    else:
        alpha = np.where(f > 0, np.minimum(r_pos[rows], r_neg[cols]), np.minimum(r_neg[rows], r_pos[cols]))
    return u_low + dt * np.add.reduceat(alpha * f, indptr[:-1]) / ml


HUBS = {"star15": 0, "hub300": 150}


def marked_rows(name):
    """node 0, node n - 1, the hub, and the rows on both sides of every seam between two row strips: where a delta in a
    Chebyshev right-hand side shows an error of the halo or of the long row (the iterate's support grows by one ring of
    neighbours per iteration)"""
    n = NODES[name]
    rows = {0, n - 1}
    if name in HUBS:
        rows.add(HUBS[name])
    if name in STRIP_ROWS:
        R = STRIP_ROWS[name]
        for s in range(R, n, R):
            rows.update((s - 1, s))
    return sorted(rows)
