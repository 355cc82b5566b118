"""The operator primitives of include/femfct.h, one by one, in every kernel regime (-m gpu), against the plain references
of tests/primitives_reference.py (pinned by tests/test_primitives_reference.py).

Contexts are built directly (Context + set_mesh_square / set_pattern_csr); cases that share a mesh share one context
(_context: one at a time, closed when the key changes).  N is the number of nodes per side of the unit square.  Every
Chebyshev case asserts the regime it claims (femfct_kernel_regime, femfct_patch_walkers, femfct_launch_info) unless a
tuning knob of regime_helpers.REGIME_KNOBS is set in the environment; the comparisons hold whatever the knobs say.

Bars ("Bars of the primitives' tests"): u = 2^-53.
  Chebyshev       relative l2 < 1e-13 per member against the longdouble recurrence (the bar of test_gpu_step.py and
                  test_gpu_edge.py); batched member vs the same member alone < 1e-12 (MEMBER_TOL of the regimes test)
  spmv            |y_i - ref_i| <= (W + 2) u (|alpha| sum_j |a_ij x_j| + |beta y_i|)
  transpose, off-diagonals of D, csr <-> ell, elementwise kernels: bitwise
  diagonal of D   |d_ii + sum_j d_ij| <= (W - 1) u sum_j |d_ij|
  reductions      |got - ref| <= d u S_abs, d counted from the code (reduction_depth)
  drift rhs       |got_i - ref_i| <= 16 u S_abs_i
  BiCGStab        rel < 1e-10 against spsolve, solver_resid <= 1e-13 (the bars of test_bicgstab_vs_spsolve)
"""
import importlib
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import spsolve

import generic_patterns as gp
import primitives_reference as pr
from regime_helpers import REGIME_KNOBS, nine_point_problem, regime_knobs_default

pytestmark = pytest.mark.gpu

U = pr.U
MEMBER_TOL = 1e-12
CHEB_TOL = 1e-13


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _report(family, case, **figs):
    print(f"[primitives] {family} {case}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}"
                                                          for k, v in figs.items()))


# ------------------------------------------------------------------------------------------------ contexts
class Pat:
    """A context with its pattern as CSR arrays (sorted columns), read back from the ELL columns of the device."""

    def __init__(self, hp, ctx, N=None, order=None):
        self.hp, self.ctx, self.N, self.order = hp, ctx, N, order
        self.n, self.W = ctx.n, ctx.W
        self.cols = ctx.ell_cols().astype(np.int64)                      # (W, n)
        n, W = self.n, self.W
        rows = np.broadcast_to(np.arange(n), (W, n))
        keep = np.ones((W, n), dtype=bool)
        keep[1:] = self.cols[1:] != rows[1:]                             # padding slots name their own row
        key = np.unique(rows[keep] * n + self.cols[keep])
        self.indices = (key % n).astype(np.int32)
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int32)
        self.nnz = self.indices.size
        self._mass = self._oracle = None

    @property
    def pattern(self):
        return self.indptr, self.indices

    def device_mass(self):
        """the registered mass matrix, CSR values"""
        if self._mass is None:
            self._mass = self.ctx.ell_to_csr(self.ctx.mass_ell, self.nnz)
        return self._mass

    def oracle(self):
        """(mesh, dof[nt, 3], longdouble geometry) of the oracle's mesh in this context's node numbering, after checking the
        registered mass matrix against the oracle's assembly (whose coordinate differences cost it about N u, see
        primitives_reference.p1_geometry; the references below take the registered matrix as the operation's input)"""
        if self._oracle is None:
            from oracle.mesh import SquareMesh
            from oracle.assembly import P1Assembler
            mesh = SquareMesh(0.0, 1.0, self.N - 1)
            asm = P1Assembler(mesh)
            M = asm.mass()
            if self.order == self.hp.ORDER_VERTEX:
                v2d = mesh.vertex_to_dof
                M, dof = M[v2d][:, v2d], mesh.cells
            else:
                dof = asm.dof
            M = csr_matrix(M)
            M.sort_indices()
            assert np.array_equal(M.indptr, self.indptr) and np.array_equal(M.indices, self.indices)
            assert np.all(np.abs(self.device_mass() - M.data) <= 4 * self.N * U * np.abs(M.data))
            self._oracle = (mesh, dof, pr.p1_geometry(mesh))
        return self._oracle

    def diagonal(self, vals):
        return csr_matrix((vals, self.indices, self.indptr), shape=(self.n, self.n)).diagonal()

    def node(self, ix, iy):
        v = min(iy, self.N - 1) * self.N + min(ix, self.N - 1)
        return v if self.order == self.hp.ORDER_VERTEX else int(self.oracle()[0].vertex_to_dof[v])

    def ell(self, vals):
        return pr.ell_layout(self.cols, self.indptr, self.indices, vals)

    def upload_mats(self, vals):
        """(B, nnz) CSR values -> one device array of B ELL matrices"""
        vals = np.atleast_2d(vals)
        wn = self.W * self.n
        big = self.ctx.empty(vals.shape[0] * wn)
        for b, v in enumerate(vals):
            self.ctx.csr_to_ell(v, out=big.ptr + 8 * b * wn)
        return big


_CTX = {}


def _context(hp, monkeypatch, kind, N, order=None, env=None, fusion=None):
    """The module's one live context: mesh (set_mesh_square on the unit square), the width-9 generic pattern, or one of
    tests/generic_patterns.py with N its name."""
    env = dict(env or {})
    key = (kind, N, order, tuple(sorted(env.items())), fusion, tuple(os.environ.get(k) for k in REGIME_KNOBS))
    if key not in _CTX:
        for p in _CTX.values():
            p.ctx.close()
        _CTX.clear()
        for k, v in env.items():
            monkeypatch.setenv(k, v)                 # read when the context is created
        ctx = hp.Context(0)
        if kind == "mesh":
            ctx.set_mesh_square(0.0, 1.0, N - 1, order)
        else:
            M, _ = nine_point_problem(N, np.random.default_rng(N)) if kind == "nine" else gp.matrices(N)
            M.sort_indices()
            ctx.set_pattern_csr(M.indptr, M.indices)
            ctx.set_mass(M.data, np.asarray(M.sum(axis=1)).ravel())
        if fusion is not None:
            ctx.set_fusion(*fusion)
        _CTX[key] = Pat(hp, ctx, N, order)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _CTX.values():
        p.ctx.close()
    _CTX.clear()


class Dev:
    """device arrays of one test, freed at its end"""

    def __init__(self, ctx):
        self.ctx, self.arrs = ctx, []

    def __call__(self, host):
        a = self.ctx.array(np.ascontiguousarray(host, dtype=np.float64).ravel())
        self.arrs.append(a)
        return a

    def empty(self, count, fill=None):
        a = self.ctx.empty(count)
        if fill is not None:
            a.upload(np.full(count, fill))
        self.arrs.append(a)
        return a

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.arrs:
            a.free()


def spread(rng, *shape):
    """mixed sign, magnitudes spread over 1e-3 .. 1e3"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)


# ------------------------------------------------------------------------------------------------ Chebyshev
# Iterations per launch: 8 on the row strips (StripPlan.K), 10 on the 32-patch tiles (femfct_tile_plan without a budget),
# 8 .. 10 on the 64-patch kernels (femfct_tile4_halo picks it per iteration count: 9 -> 9, 10 -> 10, 11 -> 8 + 3,
# 20 -> 10 + 10, 21 -> 8 + 8 + 5), 24 on the single patch.  femfct_launch_info reports the halo of a Jacobi launch only,
# which a stand-alone femfct_chebsi never makes, so the counts 1, 2, 3, H - 1, H, H + 1, 20, 2 H + 1 are taken for
# every H of 8 .. 10 at once; on the single patch 23, 24, 25 and 49 (one launch, one launch, 24 + 1, 24 + 24 + 1).
COUNTS = (1, 2, 3, 7, 8, 9, 10, 11, 17, 19, 20, 21)
COUNTS_SINGLE = (1, 2, 3, 20, 23, 24, 25, 49)
SPECTRA = ((0.5, 2.0), (0.25, 3.0))

CHEB_CASES = [
    # id, N, order, B, env, fusion, regime, interior patches of the split launch (None: not asked), walkers
    pytest.param(46, "FENICS", 3, {}, (False, False), "ROWS", None, 0, id="rows-N46-B3"),
    pytest.param(46, "FENICS", 3, {}, (True, False), "STRIPS", None, 0, id="strips-N46-B3"),
    pytest.param(46, "VERTEX", 1, {}, None, "TILE32", None, 0, id="tile32-N46-B1"),
    pytest.param(61, "VERTEX", 1, {}, None, "TILE32", None, 0, id="tile32-N61-B1"),
    pytest.param(61, "VERTEX", 5, {}, None, "TILE32", None, 0, id="tile32-N61-B5"),
    pytest.param(81, "VERTEX", 14, {}, None, "PATCH64", 0, 0, id="patch64-N81-B14-partial-edge"),
    pytest.param(301, "VERTEX", 6, {}, None, "PATCH64", "split", 0, id="patch64-N301-B6-interior-ring"),
    # (five "compute units": 49 patches would take the interior / ring split first, so that one is switched off here)
    pytest.param(301, "VERTEX", 1, {"FEMFCT_T4_WALKERS": "5", "FEMFCT_T4_INT": "0"}, None, "PATCH64", 0, 5,
                 id="patch64-N301-B1-walkers5"),
    pytest.param(47, "VERTEX", 8, {"FEMFCT_TILE4": "2"}, None, "PATCH64", 0, 0, id="single-patch-N47-B8"),
]


def _cheb_rhs(P, B, seed):
    """a random vector plus deltas at a corner node, at nodes on the seams of the 12-, 44- and 48-node tiles and at the
    last node: the exact iterate's support grows by one ring per iteration, so a halo error shows.  Own data per member."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((B, P.n))
    for m in range(B):
        for (ix, iy) in ((0, 0), (12, 12), (11, 24), (44, 43), (48, 47), (P.N - 1, 0)):
            b[m, P.node(ix, iy)] += 40.0 + 10.0 * m
        b[m, P.n - 1] -= 55.0
    return b


@pytest.mark.parametrize("spectrum", SPECTRA, ids=lambda s: f"l{s[0]}-{s[1]}")
@pytest.mark.parametrize("N, order, B, env, fusion, regime, interior, walkers", CHEB_CASES)
def test_chebsi_every_regime_and_launch_split(hp, monkeypatch, N, order, B, env, fusion, regime, interior, walkers, spectrum):
    """femfct_chebsi for every iteration count around the launch splits of for_cheb_launches (a launch of exactly one
    iteration writes y_out without an `old` output), two spectra, B members with their own right-hand sides: each member
    against the longdouble recurrence (< 1e-13 relative l2) and against itself run alone at batch 1 (< 1e-12)."""
    P = _context(hp, monkeypatch, "mesh", N, getattr(hp, "ORDER_" + order), env, fusion)
    ctx = P.ctx
    single = env.get("FEMFCT_TILE4") == "2"
    counts = COUNTS_SINGLE if single else COUNTS
    lmin, lmax = spectrum
    P.oracle()
    Mdata = P.device_mass()
    md = P.diagonal(Mdata)
    b = _cheb_rhs(P, B, N + B)
    refs = [pr.chebsi_iterates(*P.pattern, Mdata, md, b[m], counts, lmin, lmax) for m in range(B)]
    worst, worst_one, checked = 0.0, 0.0, regime_knobs_default()
    with Dev(ctx) as dev:
        d_b, d_y, d_y1 = dev(b), dev.empty(B * P.n), dev.empty(P.n)
        d_b1 = [dev(b[m]) for m in range(B)] if B > 1 else []
        if checked:
            assert ctx.kernel_regime(B) == getattr(hp._lib, "REGIME_" + regime)
        for k in counts:
            d_y.upload(np.full(B * P.n, np.nan))
            ctx.chebsi(d_b, d_y, k, lmin, lmax, batch=B)
            got = d_y.download().reshape(B, P.n)
            if checked and regime == "PATCH64":
                info = ctx.launch_info()
                assert ctx.patch_walkers(B, k) == walkers, (k, ctx.patch_walkers(B, k))
                assert (info["cheb_interior_patches"] > 0) == (interior == "split"), (k, info)
            for m in range(B):
                e = rel(got[m], refs[m][k])
                worst = max(worst, e)
                assert e < CHEB_TOL, (k, m, e)
                if B > 1:
                    ctx.chebsi(d_b1[m], d_y1, k, lmin, lmax, batch=1)
                    e1 = rel(got[m], d_y1.download())
                    worst_one = max(worst_one, e1)
                    assert e1 < MEMBER_TOL, (k, m, e1)
    _report("chebsi", f"{regime} N={N} B={B} {order.lower()} env={env} lmin={lmin} lmax={lmax}", counts=list(counts),
            worst_vs_longdouble=worst, bar=CHEB_TOL, worst_vs_alone=worst_one, bar_alone=MEMBER_TOL)


@pytest.mark.parametrize("spectrum", SPECTRA, ids=lambda s: f"l{s[0]}-{s[1]}")
def test_chebsi_md_row_kernels(hp, monkeypatch, spectrum):
    """femfct_chebsi_md: the same counts on the one-sweep row kernels with a perturbed preconditioner diagonal;
    batch = 2 is an argument error."""
    P = _context(hp, monkeypatch, "mesh", 46, hp.ORDER_FENICS, {}, (False, False))
    ctx = P.ctx
    lmin, lmax = spectrum
    P.oracle()
    Mdata = P.device_mass()
    rng = np.random.default_rng(46)
    md = P.diagonal(Mdata) * (1.0 + 0.3 * rng.random(P.n))
    b = _cheb_rhs(P, 1, 7)[0]
    ref = pr.chebsi_iterates(*P.pattern, Mdata, md, b, COUNTS, lmin, lmax)
    worst = 0.0
    with Dev(ctx) as dev:
        d_b, d_md, d_y = dev(b), dev(md), dev.empty(P.n)
        for k in COUNTS:
            d_y.upload(np.full(P.n, np.nan))
            ctx.chebsi_md(d_b, d_y, d_md, k, lmin, lmax)
            e = rel(d_y.download(), ref[k])
            worst = max(worst, e)
            assert e < CHEB_TOL, (k, e)
        d_b2, d_y2 = dev(np.tile(b, 2)), dev.empty(2 * P.n)
        with pytest.raises(ValueError):
            ctx.chebsi_md(d_b2, d_y2, d_md, 7, lmin, lmax, batch=2)
    _report("chebsi_md", f"ROWS N=46 fenics lmin={lmin} lmax={lmax}", worst_vs_longdouble=worst, bar=CHEB_TOL)


# ------------------------------------------------------------------------------------------------ matrix helpers
PATTERNS = [pytest.param("mesh", N, o, id=f"{o.lower()}-N{N}") for o in ("VERTEX", "FENICS") for N in (2, 9, 46)] + \
           [pytest.param("nine", 6, None, id="nine-point-N6")] + \
           [pytest.param("generic", name, None, id=name) for name in gp.NAMES]


def _seed(N):
    """N of a mesh, the number of nodes of a named pattern"""
    return N if isinstance(N, int) else gp.NODES[N]


def _pattern(hp, monkeypatch, kind, N, order):
    return _context(hp, monkeypatch, kind, N, None if order is None else getattr(hp, "ORDER_" + order))


def _mixed(rng, B, nnz):
    """mixed signs and exact zeros"""
    k = rng.standard_normal((B, nnz))
    k[rng.random((B, nnz)) < 0.3] = 0.0
    return k


@pytest.mark.parametrize("kind, N, order", PATTERNS)
def test_csr_ell_round_trip_and_transpose(hp, monkeypatch, kind, N, order):
    """csr_to_ell -> ell_to_csr is bitwise; the raw ELL array is the CSR matrix laid out on the slots; femfct_ell_transpose
    is bitwise the scipy transpose on the pattern, applied twice it gives the input back; in == out is refused."""
    P = _pattern(hp, monkeypatch, kind, N, order)
    ctx = P.ctx
    vals = _mixed(np.random.default_rng(_seed(N)), 1, P.nnz)[0]
    A = csr_matrix((vals, P.indices, P.indptr), shape=(P.n, P.n))
    At = csr_matrix(A.T)
    At.sort_indices()
    assert np.array_equal(At.indices, P.indices)
    ell = ctx.csr_to_ell(vals)
    try:
        assert np.array_equal(ctx.ell_to_csr(ell, P.nnz), vals)
        assert np.array_equal(ell.download().reshape(P.W, P.n), P.ell(vals))
        t = ctx.ell_transpose(ell)
        tt = ctx.ell_transpose(t)
        assert np.array_equal(pr.transpose_values(*P.pattern, vals), At.data)
        assert np.array_equal(t.download().reshape(P.W, P.n), P.ell(At.data))
        assert np.array_equal(tt.download(), ell.download())
        with pytest.raises(ValueError):
            ctx.ell_transpose(ell, ell)
        t.free(); tt.free()
    finally:
        ell.free()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind, N, order", PATTERNS)
def test_spmv(hp, monkeypatch, kind, N, order, B):
    """y = alpha A x + beta y with a matrix per member; with beta = 0 a NaN-filled y must come out finite (never read)."""
    P = _pattern(hp, monkeypatch, kind, N, order)
    ctx = P.ctx
    rng = np.random.default_rng(10 * _seed(N) + B)
    vals, x, y0 = _mixed(rng, B, P.nnz), rng.standard_normal((B, P.n)), rng.standard_normal((B, P.n))
    worst = 0.0
    with Dev(ctx) as dev:
        mats = P.upload_mats(vals)
        dev.arrs.append(mats)
        d_x, d_y = dev(x), dev.empty(B * P.n)
        for alpha, beta in ((1.0, 0.0), (-2.5, 0.0), (1.0, 1.0), (0.5, -3.0)):
            yin = y0 if beta != 0.0 else np.full((B, P.n), np.nan)
            d_y.upload(yin)
            ctx.spmv(mats, d_x, d_y, alpha, beta, batch=B)
            got = d_y.download().reshape(B, P.n)
            assert np.all(np.isfinite(got)), (alpha, beta)
            for m in range(B):
                ref, scale = pr.spmv(*P.pattern, vals[m], x[m], alpha, beta, y0[m])
                err = np.abs(got[m] - ref)
                assert np.all(err <= (P.W + 2) * U * scale), (alpha, beta, m, (err / np.maximum(scale, 1e-300)).max() / U)
                worst = max(worst, float((err / np.maximum(scale, 1e-300)).max() / U))
    _report("spmv", f"{kind} N={N} {order} B={B}", worst_over_u_scale=worst, bar=P.W + 2)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind, N, order", PATTERNS)
def test_artificial_diffusion(hp, monkeypatch, kind, N, order, B):
    """D from K (mixed signs, exact zeros), a matrix per member: off-diagonals bitwise max(0, -k_ij, -k_ji) and bitwise
    symmetric, padding slots 0, diagonal -sum_j d_ij to (W - 1) u sum |d_ij|."""
    P = _pattern(hp, monkeypatch, kind, N, order)
    ctx = P.ctx
    k = _mixed(np.random.default_rng(20 * _seed(N) + B), B, P.nnz)
    wn = P.W * P.n
    worst = 0.0
    with Dev(ctx) as dev:
        K = P.upload_mats(k)
        dev.arrs.append(K)
        D = dev.empty(B * wn, fill=np.nan)
        ctx.artificial_diffusion(K, D, batch=B)
        got = D.download().reshape(B, P.W, P.n)
        for m in range(B):
            d = pr.artificial_diffusion_offdiag(*P.pattern, k[m])
            assert np.array_equal(got[m, 1:], P.ell(d)[1:])                      # off-diagonals; padding slots hold 0
            csr = ctx.ell_to_csr(D.ptr + 8 * m * wn, P.nnz)
            off = pr.rows_of(P.indptr) != P.indices
            assert np.array_equal(csr[off], pr.transpose_values(*P.pattern, csr)[off])
            s = got[m, 1:].astype(pr.LD).sum(axis=0)
            sabs = np.abs(got[m, 1:]).astype(pr.LD).sum(axis=0)
            err = np.abs(got[m, 0].astype(pr.LD) + s).astype(np.float64)
            assert np.all(err <= (P.W - 1) * U * sabs.astype(np.float64)), m
            nz = sabs > 0
            if nz.any():
                worst = max(worst, float((err[nz] / sabs[nz].astype(np.float64)).max() / U))
    _report("artificial_diffusion", f"{kind} N={N} {order} B={B}", diag_worst_over_u_sumabs=worst, bar=P.W - 1)


# ------------------------------------------------------------------------------------------------ reductions
def reduction_depth(n, W, levels, accumulates):
    """d: the longest chain of rounded operations between a product phi_i M_ij phi_j and the result, from the code.

    k_quadform (kernels_pgd.hip), launched with femfct_geom (kernels_step.hip): blocks of bs = 64 threads up to n = 65536,
    else 256; G = min(ceil(n / bs), 2048) blocks; block_rows gives each ceil(n / G) rows rounded up to 64, so a thread owns
    R = ceil(chunk / bs) rows (R = 1 below the cap, 2 at n = 525 625, where the trailing blocks own nothing).
        2       the products M_ij * phi_j and phi_i * acc
        W - 1   row accumulation acc += ...
        R       s += phi_i * acc over the thread's rows
        6       butterfly steps of wave_reduce
        bs/64-1 fold of the waves' results in block_reduce (from 0.0: the first add is exact)
    k_reduce_levels, one block of 256 threads per member over levels * G partials (w * partial is exact):
        L       = ceil(levels * G / 256) adds of the per-thread loop
        6 + 3   its butterflies and its fold of four waves
        1       scale * s
    and one add for every later accumulate into the same result (femfct_cost_functional: + var2 misfit, + control term)."""
    bs = 64 if n <= 65536 else 256
    G = max(1, min(-(-n // bs), 2048))
    chunk = -(-(-(-n // G)) // 64) * 64
    R = -(-chunk // bs)
    L = -(-(levels * G) // 256)
    return 2 + (W - 1) + R + 6 + (bs // 64 - 1) + L + 6 + 3 + 1 + accumulates


REDUCTION_CASES = [pytest.param(N, Nt, B, id=f"N{N}-Nt{Nt}-B{B}")
                   for N in (2, 8, 9) for Nt in (1, 2, 5) for B in (1, 3)] + \
                  [pytest.param(N, 1, 1, id=f"N{N}-Nt1-B1") for N in (256, 257, 725)]


@pytest.mark.parametrize("N, Nt, B", REDUCTION_CASES)
def test_reductions(hp, monkeypatch, N, Nt, B):
    """femfct_l2_norm_sq_Q / _Omega with and without b, femfct_cost_functional all-time and final-time with and without
    var2, every member with its own states, targets and controls (a wrong stride picks up another member's data):
    |got - ref| <= d u S_abs with the exactly summed reference, d = reduction_depth(...) (derived, see there; the
    measured ratio is printed beside it).  n = 4, 64, 81 (less than a wave, exactly one chunk, one chunk and a bit),
    65 536 / 66 049 (both sides of the 64 -> 256 thread switch) and 525 625 (past the 2048-block cap)."""
    P = _context(hp, monkeypatch, "mesh", N, hp.ORDER_VERTEX)
    ctx, n = P.ctx, P.n
    csr = (P.indptr, P.indices, P.device_mass())
    rng = np.random.default_rng(1000 * N + 10 * Nt + B)
    tl = (Nt + 1) * n
    v1, t1, v2, t2, c = (spread(rng, B, tl) for _ in range(5))
    dt, beta = 0.013, 0.37
    figs = {}

    def check(name, got, ref, levels, acc):
        d = reduction_depth(n, P.W, levels, acc)
        for m in range(B):
            val, sabs = ref(m)
            ratio = abs(pr.LD(got[m]) - val) / (U * sabs)
            figs[name] = max(figs.get(name, 0.0), float(ratio))
            figs["d_" + name] = d
            assert ratio <= d, (name, m, float(ratio), d)

    with Dev(ctx) as dev:
        d_v1, d_t1, d_v2, d_t2, d_c = (dev(a) for a in (v1, t1, v2, t2, c))
        d_tf1, d_tf2 = dev(t1[:, :n]), dev(t2[:, :n])                       # final-time targets: n values per member
        d_o1, d_oa, d_ob = dev(c[:, :n]), dev(v1[:, :n]), dev(t1[:, :n])     # level 0 of c, v1, t1: n values per member
        check("Q", ctx.l2_norm_sq_Q(d_c, None, Nt, dt, batch=B), lambda m: pr.norm_sq_Q(csr, c[m], None, Nt, dt), Nt + 1, 0)
        check("Q_b", ctx.l2_norm_sq_Q(d_v1, d_t1, Nt, dt, batch=B), lambda m: pr.norm_sq_Q(csr, v1[m], t1[m], Nt, dt), Nt + 1, 0)
        check("Omega", ctx.l2_norm_sq_Omega(d_o1, None, batch=B), lambda m: pr.norm_sq_Omega(csr, c[m, :n], None), 1, 0)
        check("Omega_b", ctx.l2_norm_sq_Omega(d_oa, d_ob, batch=B), lambda m: pr.norm_sq_Omega(csr, v1[m, :n], t1[m, :n]), 1, 0)
        check("J_all", ctx.cost_functional(d_v1, d_t1, d_c, Nt, dt, beta, "alltime", batch=B),
              lambda m: pr.cost(csr, v1[m], t1[m], c[m], Nt, dt, beta, "alltime"), Nt + 1, 1)
        check("J_all_2", ctx.cost_functional(d_v1, d_t1, d_c, Nt, dt, beta, "alltime", var2=d_v2, var2_target=d_t2, batch=B),
              lambda m: pr.cost(csr, v1[m], t1[m], c[m], Nt, dt, beta, "alltime", v2[m], t2[m]), Nt + 1, 2)
        check("J_fin", ctx.cost_functional(d_v1, d_tf1, d_c, Nt, dt, beta, "finaltime", batch=B),
              lambda m: pr.cost(csr, v1[m], t1[m, :n], c[m], Nt, dt, beta, "finaltime"), Nt + 1, 1)
        check("J_fin_2", ctx.cost_functional(d_v1, d_tf1, d_c, Nt, dt, beta, "finaltime", var2=d_v2, var2_target=d_tf2, batch=B),
              lambda m: pr.cost(csr, v1[m], t1[m, :n], c[m], Nt, dt, beta, "finaltime", v2[m], t2[m, :n]), Nt + 1, 2)
    _report("reductions", f"N={N} n={n} Nt={Nt} B={B} |got-ref|/(u S_abs) beside d", **figs)


def test_reduction_argument_errors(hp, monkeypatch):
    """each is refused before any launch: levels * batch > 65535, var2 without var2_target, num_steps = 0 for the cost"""
    P = _context(hp, monkeypatch, "mesh", 9, hp.ORDER_VERTEX)
    ctx, n = P.ctx, P.n
    with Dev(ctx) as dev:
        a = dev(np.ones(3 * n))
        with pytest.raises(ValueError):
            ctx.l2_norm_sq_Q(a, None, 65535, 0.1, batch=1)
        with pytest.raises(ValueError):
            ctx.l2_norm_sq_Q(a, None, 21845, 0.1, batch=3)
        with pytest.raises(ValueError):
            ctx.cost_functional(a, a, a, 21845, 0.1, 0.1, "alltime", batch=3)
        with pytest.raises(ValueError):
            ctx.cost_functional(a, a, a, 2, 0.1, 0.1, "alltime", var2=a, var2_target=None)
        with pytest.raises(ValueError):
            ctx.cost_functional(a, a, a, 0, 0.1, 0.1, "alltime")


# ------------------------------------------------------------------------------------------------ elementwise kernels
COUNTS_EW = (0, 1, 255, 256, 257, 4096 * 256 + 3)           # the last one enters the grid-stride loop (4096 x 256 threads)
SENTINEL = -7.25


def _ew_data(count, seed):
    rng = np.random.default_rng(seed)
    c, d, g = rng.standard_normal(count), rng.standard_normal(count), rng.standard_normal(count)
    c[::7], d[::7] = -0.4, 0.0                 # ties exactly at the lower bound ...
    c[3::7], d[3::7] = 0.6, 0.0                # ... and at the upper one
    return c, d, g


@pytest.mark.parametrize("count", COUNTS_EW)
def test_elementwise_kernels_bitwise(hp, monkeypatch, count):
    """project_control (clipped on both sides, ties at the bounds, out aliasing c as femfct.h promises), axpby with and
    without b, descent_pointwise in both forms: bitwise the NumPy expression, nothing written past `count`."""
    P = _context(hp, monkeypatch, "mesh", 9, hp.ORDER_VERTEX)
    ctx = P.ctx
    c, d, g = _ew_data(count, count)
    s, lo, hi = 0.5, -0.4, 0.6
    pad = count + 5

    def padded(a):
        return np.concatenate([a, np.full(pad - count, SENTINEL)])

    with Dev(ctx) as dev:
        d_c, d_d, d_g, out = dev(padded(c)), dev(padded(d)), dev(padded(g)), dev.empty(pad)

        def run(call, ref):
            out.upload(np.full(pad, SENTINEL))
            call()
            got = out.download()
            assert np.array_equal(got[:count], ref) and np.all(got[count:] == SENTINEL)
            return got[:count]

        ref = pr.clip_axpy(c, s, d, lo, hi)
        if count > 7:
            assert (ref == lo).sum() > count // 7 and (ref == hi).sum() > count // 8 and ((ref > lo) & (ref < hi)).any()
        plain = run(lambda: ctx.project_control(d_c, s, d_d, lo, hi, out, count), ref)
        out.upload(padded(c))                                    # out aliases c
        ctx.project_control(out, s, d_d, lo, hi, out, count)
        got = out.download()
        assert np.array_equal(got[:count], plain) and np.all(got[count:] == SENTINEL)
        run(lambda: ctx.axpby(count, -1.5, d_c, 0.75, d_d, out), pr.axpby(-1.5, c, 0.75, d))
        run(lambda: ctx.axpby(count, -1.5, d_c, 0.75, None, out), pr.axpby(-1.5, c, 0.75, None))
        run(lambda: ctx.descent_pointwise(count, 0.1, d_c, d_d, out, y=d_g, divisor=0.3), pr.descent_pointwise(0.1, c, d, y=g, divisor=0.3))
        run(lambda: ctx.descent_pointwise(count, 0.1, d_c, d_d, out, scale=7.0), pr.descent_pointwise(0.1, c, d, scale=7.0))


@pytest.mark.parametrize("count, K", [(cnt, K) for cnt in COUNTS_EW for K in (1, 16) if not (K == 16 and cnt > 1000)])
def test_source_trials_bitwise(hp, monkeypatch, count, K):
    """femfct_source_trials with and without g and src_out: c_out[t] = clip(c + s_t d), src_out[t] = g + c_out[t]."""
    P = _context(hp, monkeypatch, "mesh", 9, hp.ORDER_VERTEX)
    ctx = P.ctx
    c, d, g = _ew_data(count, count + K)
    s0, lo, hi = 0.8, -0.4, 0.6
    with Dev(ctx) as dev:
        d_c, d_d, d_g = dev(np.append(c, 0.0)), dev(np.append(d, 0.0)), dev(np.append(g, 0.0))
        c_out, src_out = dev.empty(K * count + 1), dev.empty(K * count + 1)
        for with_g in (True, False):
            for with_src in (True, False):
                c_out.upload(np.full(K * count + 1, SENTINEL))
                src_out.upload(np.full(K * count + 1, SENTINEL))
                ctx.source_trials(d_c, d_d, s0, K, lo, hi, count, c_out, src_out if with_src else None, d_g if with_g else None)
                rc, rs = pr.source_trials(c, d, g if with_g else None, s0, K, lo, hi)
                gc, gs = c_out.download(), src_out.download()
                assert np.array_equal(gc[:-1], rc.ravel()) and gc[-1] == SENTINEL
                assert np.array_equal(gs[:-1], rs.ravel() if with_src else np.full(K * count, SENTINEL)) and gs[-1] == SENTINEL


# ------------------------------------------------------------------------------------------------ drift right-hand side
@pytest.mark.parametrize("N", [2, 3, 13])
@pytest.mark.parametrize("order", ["VERTEX", "FENICS"])
def test_drift_gradient_rhs_raw(hp, monkeypatch, order, N):
    """femfct_drift_gradient_rhs before any Chebyshev smoothing, row by row -- corner and boundary rows visit 1, 2 or 3
    triangles (N = 2: every node is a corner): levels 1 and 4, drifts with bx != by, beta 0 and 0.1, random u, p, c, and
    u linear in x with p = 1, where the integral is bx * ml_i in closed form (that case also checks the reference).
    |got_i - ref_i| <= 16 u S_abs_i: 7 mass terms, 6 triangles, scale, generously."""
    P = _context(hp, monkeypatch, "mesh", N, getattr(hp, "ORDER_" + order))
    ctx, n = P.ctx, P.n
    mesh, dof, geom = P.oracle()
    Mdata = P.device_mass()
    ml = pr.lumped_mass(geom, dof, n)
    xs = mesh.x if order == "VERTEX" else mesh.x[mesh.dof_to_vertex]
    rng = np.random.default_rng(N)
    worst = 0.0
    with Dev(ctx) as dev:
        for levels in (1, 4):
            c, u, p = (rng.standard_normal((levels, n)) for _ in range(3))
            u[-1], p[-1] = xs, 1.0                                     # the closed-form level
            d_c, d_u, d_p, out = dev(c), dev(u), dev(p), dev.empty(levels * n)
            for drift in ((1.0, 1.0), (0.7, -1.3), (0.0, 1.0)):
                for beta in (0.0, 0.1):
                    out.upload(np.full(levels * n, np.nan))
                    ctx.drift_gradient_rhs(d_c, d_u, d_p, beta, out, levels, drift=drift)
                    got = out.download().reshape(levels, n)
                    for lv in range(levels):
                        ref, sabs = pr.drift_rhs(geom, dof, *P.pattern, Mdata, c[lv], u[lv], p[lv], beta, drift)
                        if lv == levels - 1:       # closed form; the nodal x = fl(i h) carry u each, 1 / h of it in grad u
                            mc = pr.matvec(*P.pattern, Mdata, c[lv])[0]
                            closed = -(pr.LD(beta) * mc + pr.LD(drift[0]) * ml)
                            assert np.all(np.abs(ref - closed.astype(np.float64)) <= (N + 1) * U * sabs)
                        err = np.abs(got[lv] - ref)
                        ratio = float((err / np.maximum(sabs, 1e-300)).max() / U)
                        assert np.all(err <= 16 * U * sabs), (levels, drift, beta, lv, ratio)
                        worst = max(worst, ratio)
    _report("drift_gradient_rhs", f"{order.lower()} N={N}", worst_over_u_sabs=worst, bar=16)


# ------------------------------------------------------------------------------------------------ BiCGStab
def test_bicgstab_batched(hp):
    """The two matrices of test_bicgstab_vs_spsolve at N = 41 with three right-hand sides and a non-zero x0: once with a
    matrix per member (scaled copies), once with mat_shared.  rel < 1e-10 against spsolve, solver_resid <= 1e-13."""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    from oracle.traj import schnak_wind
    mesh = SquareMesh(0.0, 1.0, 40)
    asm = P1Assembler(mesh)
    n, B = mesh.nodes, 3
    rng = np.random.default_rng(1)
    M, Ad = asm.mass(), asm.stiffness()
    A = asm.convection(schnak_wind)
    u = 1 + 0.2 * rng.random(n)
    mats = [M + 1e-3 * (8.6676 * Ad - 0.6 * A + 230.82 * asm.weighted_mass(lambda at: at(u) ** 2)),   # helpers.py:595
            M + 1e-3 * (0.05 * Ad + 100 * M)]                                                            # helpers.py:1308
    _bicgstab_batched(hp, M, mats, "N=41", rng)


def _bicgstab_batched(hp, M, mats, label, rng, B=3):
    """the body of test_bicgstab_batched for a mass matrix (pattern) M and matrices `mats` on its pattern"""
    n = M.shape[0]
    ctx = hp.Context(0)
    try:
        Mc = csr_matrix(M).copy()
        Mc.sort_indices()
        ctx.set_pattern_csr(Mc.indptr, Mc.indices)
        ctx.set_mass(Mc.data, np.asarray(M.sum(axis=1)).ravel())
        P = Pat(hp, ctx)
        for k, Mat in enumerate(mats):
            Mat = Mat.tocsr()
            Mat.sort_indices()
            b, x0 = rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, n))
            for shared in (False, True):
                scales = (1.0, 1.0, 1.0) if shared else (1.0, 1.5, 0.75)
                with Dev(ctx) as dev:
                    ell = P.upload_mats(Mat.data[None] if shared else np.stack([sc * Mat.data for sc in scales]))
                    dev.arrs.append(ell)
                    x = dev.empty(B * n, fill=np.nan)
                    info = ctx.bicgstab(ell, dev(b), dev(x0), x, batch=B, mat_shared=shared)
                    got = x.download().reshape(B, n)
                worst = 0.0
                for m in range(B):
                    xs = spsolve((scales[m] * Mat).tocsc(), b[m])
                    worst = max(worst, rel(got[m], xs))
                    assert rel(got[m], xs) < 1e-10, (k, shared, m, info)
                    assert info[m]["solver_resid"] <= 1e-13, (k, shared, m, info)
                _report("bicgstab", f"{label} matrix={k} B={B} mat_shared={shared}", worst_vs_spsolve=worst, bar=1e-10,
                        worst_resid=max(i["solver_resid"] for i in info), bar_resid=1e-13)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", gp.NAMES)
def test_bicgstab_batched_generic_patterns(hp, name):
    """The same on the patterns of tests/generic_patterns.py, with the two non-symmetric matrices a step on them meets:
    M + dt A and the low-order operator M_L + dt (A - D + 0.05 M).  Same bars."""
    P = gp.problem(name, 1)
    indptr, indices = P.M.indptr, P.M.indices
    a, m = P.A[0].data, P.M.data
    diag = pr.rows_of(indptr) == indices
    d = pr.artificial_diffusion_offdiag(indptr, indices, -a)
    d[diag] = -np.add.reduceat(d, indptr[:-1])
    low = P.dt * (a - d + 0.05 * m)
    low[diag] += P.ml
    mats = [csr_matrix((v, indices, indptr), shape=P.M.shape) for v in (m + P.dt * a, low)]    # stored zeros stay stored
    _bicgstab_batched(hp, P.M, mats, name, np.random.default_rng(gp.NODES[name]))
