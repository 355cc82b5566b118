"""Plain references of the operator primitives of include/femfct.h (a helper, not a test).

Everything is written against CSR arrays (indptr, indices, data; sorted columns, full diagonal), so it depends neither
on the device's ELL layout nor on oracle/ -- tests/test_primitives_reference.py pins it against both the oracle and the
reference's own outputs before tests/test_gpu_primitives.py trusts it.  Three kinds of reference:

  * np.longdouble (64-bit mantissa, asserted below), rounded to float64 only at the end: matrix-vector product,
    Chebyshev recurrence (helpers.py:143-185), drift right-hand side (element by element);
  * scalar reductions: every product phi_i M_ij phi_j is formed in longdouble (relative error 2^-63, nothing at the
    2^-53 level); its float64 part is summed exactly with math.fsum, the remainders (2^-53 of the terms) in longdouble;
    returned with S_abs, the sum of the absolute values of all terms, the scale of the device's rounding error;
  * exact operations in float64 NumPy, in the kernel's own expression order (the library is built with
    -ffp-contract=off, so these are bitwise statements).
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no 64-bit mantissa on this platform"

U = 2.0 ** -53          # unit roundoff of float64


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ patterns
def rows_of(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


def transpose_pos(indptr, indices):
    """tpos[k] = position of (j, i) for the stored entry k = (i, j) of a structurally symmetric sorted pattern"""
    rows, cols = rows_of(indptr), np.asarray(indices, dtype=np.int64)
    order = np.lexsort((rows, cols))
    if not (np.array_equal(cols[order], rows) and np.array_equal(rows[order], cols)):
        raise ValueError("pattern is not structurally symmetric")
    return order


def ell_layout(cols, indptr, indices, data):
    """CSR values on the ELL slots cols[W, n] of the device (slot 0 the diagonal, padding slots hold column = row and 0)"""
    from scipy.sparse import csr_matrix
    W, n = cols.shape
    A = csr_matrix((np.asarray(data, dtype=np.float64), indices, indptr), shape=(n, n))
    i = np.broadcast_to(np.arange(n), (W, n))
    out = np.asarray(A[i.ravel(), cols.ravel()]).reshape(W, n).copy()
    out[1:][cols[1:] == i[1:]] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ longdouble
def matvec(indptr, indices, data, x):
    """(M x, |M| |x|) in longdouble"""
    prod = ld(data) * ld(x)[np.asarray(indices)]
    ip = np.asarray(indptr[:-1], dtype=np.int64)
    return np.add.reduceat(prod, ip), np.add.reduceat(np.abs(prod), ip)


def spmv(indptr, indices, data, x, alpha, beta, y):
    """alpha M x + beta y rounded once, and the scale |alpha| sum_j |a_ij x_j| + |beta y_i| of the device's error bound"""
    s, sabs = matvec(indptr, indices, data, x)
    val = LD(alpha) * s + (LD(beta) * ld(y) if beta != 0.0 else LD(0))
    scale = abs(LD(alpha)) * sabs + (np.abs(LD(beta) * ld(y)) if beta != 0.0 else LD(0))
    return val.astype(np.float64), scale.astype(np.float64)


def chebsi_iterates(indptr, indices, data, md, b, counts, lmin=0.5, lmax=2.0):
    """{k: y_k for k in counts} of ChebSI(b, M, md, k, lmin, lmax), helpers.py:143-185: the iterates do not depend on the
    number of iterations asked for, so one recurrence serves every count.  omega_k from oracle.fct.chebsi_omegas."""
    from oracle.fct import chebsi_omegas
    counts = sorted(set(int(k) for k in counts))
    om = chebsi_omegas(counts[-1], lmin, lmax)
    b = ld(b)
    mdl = (LD(lmin) + LD(lmax)) / 2 * ld(md)
    y_mid, y_old, out = np.zeros_like(b), np.zeros_like(b), {}
    for k in range(1, counts[-1] + 1):
        r = b - matvec(indptr, indices, data, y_mid)[0]
        y_new = LD(om[k - 1]) * (r / mdl + y_mid - y_old) + y_old
        y_old, y_mid = y_mid, y_new
        if k in counts:
            out[k] = y_new.astype(np.float64)
    return out


def p1_geometry(mesh):
    """(grad[nt, 3, 2], MK[nt, 3, 3], area[nt]) of oracle.assembly.P1Assembler -- its formulas, evaluated in longdouble on
    the exact vertex coordinates a1 + i h, h = (a2 - a1) / n_cells.  (The assembler's own float64 arrays carry the
    cancellation of its coordinate differences, a relative error of about n_cells * 2^-53: too coarse to measure a
    kernel to a few units of 2^-53 against.)"""
    h = (LD(mesh.a2) - LD(mesh.a1)) / mesh.n_cells
    c = mesh.cells
    xl, yl = LD(mesh.a1) + mesh.ix.astype(LD) * h, LD(mesh.a1) + mesh.iy.astype(LD) * h
    x = np.stack([xl[c], yl[c]], axis=2)
    e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = np.abs(det) / 2
    g = np.empty((c.shape[0], 3, 2), dtype=LD)
    g[:, 1, 0], g[:, 1, 1] = e2[:, 1] / det, -e2[:, 0] / det
    g[:, 2, 0], g[:, 2, 1] = -e1[:, 1] / det, e1[:, 0] / det
    g[:, 0] = -(g[:, 1] + g[:, 2])
    MK = (area[:, None, None] / 12) * (np.ones((3, 3)) + np.eye(3)).astype(LD)[None]
    return g, MK, area


def drift_rhs(geom, dof, indptr, indices, mdata, c, u, p, beta, b):
    """-(beta M c + sum_K p-weighted b.grad u) of one time level, element by element with the P1 element matrices of
    geom = p1_geometry(mesh); dof[nt, 3] numbers the cells' nodes in the order of c, u, p (P1Assembler.dof: the FEniCS
    order, mesh.cells: the vertex order).  Returns (value, S_abs): S_abs_i sums the absolute values of the elementary
    products beta M_ij c_j and b_d u_a grad_a,d (M_K)_im p_m that make up row i."""
    mc, mcabs = matvec(indptr, indices, mdata, c)
    grad, MK = geom[0], geom[1]
    ul, pl = ld(u)[dof], ld(p)[dof]                                            # (nt, 3)
    bl = np.array([LD(b[0]), LD(b[1])])
    s = np.einsum("ta,tad,d->t", ul, grad, bl)
    sabs = np.einsum("ta,tad,d->t", np.abs(ul), np.abs(grad), np.abs(bl))
    mp = np.einsum("tim,tm->ti", MK, pl)
    mpabs = np.einsum("tim,tm->ti", np.abs(MK), np.abs(pl))
    g, gabs = np.zeros(mc.size, dtype=LD), np.zeros(mc.size, dtype=LD)
    np.add.at(g, dof.reshape(-1), (s[:, None] * mp).reshape(-1))
    np.add.at(gabs, dof.reshape(-1), (sabs[:, None] * mpabs).reshape(-1))
    val = -(LD(beta) * mc + g)
    return val.astype(np.float64), (abs(LD(beta)) * mcabs + gabs).astype(np.float64)


def lumped_mass(geom, dof, n):
    """ml_i = sum over the triangles at node i of |K| / 3, in longdouble"""
    ml = np.zeros(n, dtype=LD)
    np.add.at(ml, dof.reshape(-1), np.repeat(geom[2] / 3, 3))
    return ml


# ------------------------------------------------------------------------------------------------ exact sums
_QUADFORMS = {}     # the modes of one reduction case share levels: (matrix, level) -> result, a few entries


def quadform(indptr, indices, data, phi):
    """(phi^T M phi, sum_ij |phi_i M_ij phi_j|) as longdoubles holding the exactly summed products"""
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    key = (np.asarray(data).size, hash(np.asarray(data).tobytes()), phi.size, hash(phi.tobytes()))
    if key not in _QUADFORMS:
        if len(_QUADFORMS) >= 16:
            _QUADFORMS.clear()
        _QUADFORMS[key] = _quadform(indptr, indices, data, phi)
    return _QUADFORMS[key]


def _quadform(indptr, indices, data, phi):
    pl = ld(phi)
    t = pl[rows_of(indptr)] * ld(data) * pl[np.asarray(indices)]
    hi = t.astype(np.float64)
    lo = t - hi.astype(LD)               # 2^-53 of the terms: their plain longdouble sum errs by 2^-63 of that
    return LD(math.fsum(hi.tolist())) + np.sum(lo), np.sum(np.abs(t))


def _levels(phi, levels):
    return np.asarray(phi, dtype=np.float64).reshape(levels, -1)


def norm_sq_Q(csr, a, b, num_steps, dt):
    """L2_norm_sq_Q(a - b), helpers.py:330-360: (value, S_abs) with the trapezoidal weights and dt folded into both"""
    phi = _levels(a, num_steps + 1) - (0.0 if b is None else _levels(b, num_steps + 1))
    w = np.ones(num_steps + 1)
    w[0] = w[-1] = 0.5            # (num_steps = 0: one level of weight 1/2, as the device's k_reduce_levels)
    q = [quadform(*csr, lv) for lv in phi]
    return (LD(dt) * sum(LD(wl) * ql[0] for wl, ql in zip(w, q)),
            abs(LD(dt)) * sum(LD(wl) * ql[1] for wl, ql in zip(w, q)))


def norm_sq_Omega(csr, a, b):
    """L2_norm_sq_Omega(a - b), helpers.py:362-381"""
    return quadform(*csr, np.asarray(a, dtype=np.float64) - (0.0 if b is None else np.asarray(b, dtype=np.float64)))


def cost(csr, var1, tgt1, control, num_steps, dt, beta, optim, var2=None, tgt2=None):
    """cost_functional, helpers.py:383-441, one member: (value, S_abs).  The scales are the float64 values the library
    forms on the host (0.5 * dt, 0.5, 0.5 * beta * dt)."""
    n = csr[0].size - 1
    val, sabs = LD(0), LD(0)
    for v, t in ((var1, tgt1), (var2, tgt2)):
        if v is None:
            continue
        if optim == "alltime":
            q, qa = norm_sq_Q(csr, v, t, num_steps, 1.0)
            sc = 0.5 * dt
        else:
            q, qa = norm_sq_Omega(csr, np.asarray(v)[num_steps * n:], t)
            sc = 0.5
        val, sabs = val + LD(sc) * q, sabs + abs(LD(sc)) * qa
    q, qa = norm_sq_Q(csr, control, None, num_steps, 1.0)
    sc = 0.5 * beta * dt
    return val + LD(sc) * q, sabs + abs(LD(sc)) * qa


# ------------------------------------------------------------------------------------------------ bitwise float64
def artificial_diffusion_offdiag(indptr, indices, k):
    """d_ij = max(0, -k_ij, -k_ji) off the diagonal, 0 on it (helpers.py:206-242; k_artdiff: fmax(0, fmax(-k, -kt)))"""
    k = np.asarray(k, dtype=np.float64)
    kt = k[transpose_pos(indptr, indices)]
    d = np.maximum(0.0, np.maximum(-k, -kt))
    d[rows_of(indptr) == np.asarray(indices)] = 0.0
    return d


def transpose_values(indptr, indices, data):
    return np.asarray(data, dtype=np.float64)[transpose_pos(indptr, indices)]


def clip_axpy(c, s, d, lo, hi):
    """update_control, helpers.py:1666-1667 (k_clip_axpy: fmin(fmax(c + s d, lo), hi))"""
    return np.minimum(np.maximum(c + s * d, lo), hi)


def axpby(alpha, a, beta, b):
    return alpha * a + (beta * b if b is not None else 0.0)


def source_trials(c, d, g, s0, K, lo, hi):
    """(c_out[K, count], src_out[K, count]) of femfct_source_trials: s_t = s0 * (1 / 2^t)"""
    c_out = np.stack([clip_axpy(c, s0 * (1.0 / float(1 << t)), d, lo, hi) for t in range(K)])
    return c_out, (1.0 * g + 1.0 * c_out if g is not None else c_out.copy())


def descent_pointwise(beta, c, x, y=None, scale=1.0, divisor=1.0):
    t = (x * y) / divisor if y is not None else scale * x
    return -(beta * c - t)
