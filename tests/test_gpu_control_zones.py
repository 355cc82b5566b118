"""GPU tests (-m gpu) of controls that are piecewise constant in space: femfct_set_control_zones / femfct_zone_restrict /
femfct_zone_prolong against NumPy (control_zones_oracle.py), the directions of ``control_space=``, and the descent loops
against the CPU loops of the same file on the set-ups of control_zones_cases.py (whose Armijo margins
test_control_zones_oracle.py checks to be >= 1e-8).

Kernel bars, derived (u = 2^-53; the references are summed in extended precision, so they carry none of it):
  * a sum of L terms in any order is within L u sum_i |y_i| of the exact sum;
  * a mass row y_i = sum_s M_is x_s of W = 7 slots (W products, W - 1 additions) is within (W + 1) u sum_s |M_is x_s|; a
    zone's sum of mass rows is therefore within L u sum_i |y_i| + (W + 1) u sum_i sum_s |M_is x_s|;
  * delta_j = sum_k Ginv_jk s_k (m products, m - 1 additions) is within (m + 1) u sum_k |Ginv_jk s_k| of the exact product
    of the same Ginv with the same (the device's) s.
The projection P = chi Ginv chi^T M with Ginv = inv(G) from the host: besides the three terms above, Ginv is not the
exact inverse of the exact G.  G's entries are sums of positive products (the P1 mass matrix has no negative entry), so
the device's G is entrywise within eps_G = (L_max + W + 1) u relative of the exact one; LAPACK's inverse X of a matrix A
satisfies |A X - I| <= c m u |A| |X| with a modest c, taken as 8: eps_inv = 8 m u.  Together
|Ginv G - I| <= kappa (eps_G + eps_inv) =: eps_P in the infinity norm, kappa = ||G|| ||Ginv||: the kappa(G) 2^-53 term.

Fold shape: N = 46 (n = 2116).  The kernel as built sums chunks of 1024 list entries per block, so the layout ``one``
there is three chunks, and ``split`` (1500 + 616 nodes) has one folded zone beside one that is not.  A table whose
largest zone has at most 256 nodes runs one wave per block, any other four: ``first256`` (256 + 185 nodes at n = 441) and
``first257`` (257 + 184) sit on either side of that threshold."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import control_intervals_cases as cc
import control_zones_cases as zc
import control_zones_oracle as czo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
W = 7


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


# ---------------------------------------------------------------------------------------------- orders and references
def to_dev(cs, a, order):
    """DoF order -> the device's order (per level)"""
    if order == 1:
        return np.array(a, dtype=np.float64)
    return np.ascontiguousarray(np.asarray(a).reshape(-1, cs["n"])[:, cs["mesh"].vertex_to_dof]).ravel()


def to_dof(cs, a, order):
    if order == 1:
        return a
    back = np.empty((a.size // cs["n"], cs["n"]))
    back[:, cs["mesh"].vertex_to_dof] = a.reshape(-1, cs["n"])
    return back.ravel()


def labels_dev(cs, lab, order):
    return lab if order == 1 else np.ascontiguousarray(lab[cs["mesh"].vertex_to_dof])


def mass_coo(ctx):
    """(rows, cols, values) of the registered mass matrix, the one femfct_zone_restrict applies: the context's own ELL
    arrays (the device assembles them itself; they agree with the oracle's to rounding, not to the bit)"""
    n, width = ctx.n, ctx.W
    assert width == W
    buf = ctx.empty(width * n)
    vals = buf.copy_from(ctx.mass_ell, width * n).download()
    buf.free()
    return np.tile(np.arange(n), width), ctx.ell_cols().ravel().astype(np.int64), vals


def extra_layout(N, name):
    if name == "split":
        lab = (np.arange(N * N) >= 1500).astype(np.int32)
        return lab, 2
    if name in ("first256", "first257"):
        lab = (np.arange(N * N) >= int(name[5:])).astype(np.int32)
        return lab, 2
    return zc.layout(N, name)


class Ref:
    """the zone operations in extended precision, with the derived bounds, in the device's order"""

    def __init__(self, lab, m, coo):
        self.lab, self.m, self.n = np.asarray(lab), m, len(lab)
        self.rows, self.cols, self.vals = coo
        self.act = self.lab >= 0
        self.sizes = np.bincount(self.lab[self.act], minlength=m)

    def zone_sum(self, y):
        out = np.zeros((y.shape[0], self.m), dtype=y.dtype)
        np.add.at(out, (slice(None), self.lab[self.act]), y[:, self.act])
        return out

    def rows_of(self, x):
        """(M x, |M| |x|) per field, extended precision"""
        x = x.reshape(-1, self.n).astype(LD)
        y, ya = np.zeros_like(x), np.zeros_like(x)
        np.add.at(y, (slice(None), self.rows), self.vals.astype(LD) * x[:, self.cols])
        np.add.at(ya, (slice(None), self.rows), np.abs(self.vals).astype(LD) * np.abs(x[:, self.cols]))
        return y, ya

    def restrict(self, x, mass):
        """(sums, bound): (fields, m) each"""
        if mass:
            y, ya = self.rows_of(x)
        else:
            y, ya = x.reshape(-1, self.n).astype(LD), None
        s = self.zone_sum(y)
        b = self.sizes[None, :] * U * self.zone_sum(np.abs(y))
        if mass:
            b = b + (W + 1) * U * self.zone_sum(ya)
        return s, b.astype(np.float64)

    def coeff(self, s, Ginv):
        """(Ginv s, bound) for the fields s (fields, m)"""
        d = s.astype(LD) @ Ginv.astype(LD).T
        b = (self.m + 1) * U * (np.abs(s).astype(LD) @ np.abs(Ginv).astype(LD).T)
        return d, b.astype(np.float64)

    def scatter(self, d):
        out = np.zeros((d.shape[0], self.n), dtype=d.dtype)
        out[:, self.act] = d[:, self.lab[self.act]]
        return out


def within(got, ref, bound, what):
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))


def check_prolonged(out, ref, what):
    """exact properties of a prolonged field: 0.0 where no control acts, one stored value per zone"""
    assert np.all(out[:, ~ref.act] == 0.0) and not np.any(np.signbit(out[:, ~ref.act])), what
    first = np.array([int(np.argmax(ref.lab == j)) for j in range(ref.m)])
    assert np.array_equal(out[:, ref.act], out[:, first][:, ref.lab[ref.act]]), what


# ---------------------------------------------------------------------------------------------- 1. the kernels
KERNEL_CASES = [(N, order, name) for N in (5, 21) for order in (0, 1)
                for name in ("quadrants", "mod3", "one", "lone") + (("each",) if N == 5 else ())]
KERNEL_CASES += [(21, 1, "first256"), (21, 0, "first257"), (46, 0, "one"), (46, 1, "split")]


@pytest.mark.parametrize("N,order,name", KERNEL_CASES, ids=[f"n{N * N}-{'fenics' if o else 'vertex'}-{nm}" for N, o, nm in KERNEL_CASES])
def test_restrict_and_prolong_vs_numpy(hp, N, order, name):
    """n = 25 and n = 441 (no multiple of 64) with 1, 7 and 41 fields, each as a batch of 3 distinct members (3, 21 and
    123 fields a call); standard normal data and magnitudes from 1e-8 to 1e8; n = 2116 for the folded sums."""
    cs = cc.sb_case(N)
    n = cs["n"]
    lab_dof, m = extra_layout(N, name)
    lab = labels_dev(cs, lab_dof, order)
    rng = np.random.default_rng(100 * N + 10 * order + len(name))
    Ginv = rng.standard_normal((m, m)) / m
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1, order)
        ref = Ref(lab, m, mass_coo(ctx))
        ctx.set_control_zones(lab, m)
        gd = ctx.array(Ginv)
        for F in ((1, 7, 41) if N < 46 else (3,)):
            for wide in (False, True):
                data = rng.standard_normal((3, F, n))
                if wide:
                    data = data * 10.0 ** rng.uniform(-8, 8, data.shape)
                x = ctx.array(data)
                s3, s1, sf, twice = ctx.zeros(3 * F * m), ctx.zeros(F * m), ctx.zeros(m), ctx.zeros(3 * F * m)
                out, o1 = ctx.zeros(3 * F * n), ctx.zeros(n)
                for mass in (False, True):
                    what = (name, F, wide, mass)
                    ctx.zone_restrict(x, 3 * F, s3, apply_mass=mass)
                    got = s3.download().reshape(3 * F, m)
                    sref, sb = ref.restrict(data, mass)
                    within(got, sref, sb, what)
                    if name == "lone" and not mass:
                        assert np.array_equal(got[:, 0], data.reshape(3 * F, n)[:, np.flatnonzero(lab == 0)[0]]), what
                    for b in range(3):                                   # a member alone: the same bits
                        ctx.zone_restrict(x.ptr + 8 * b * F * n, F, s1, apply_mass=mass)
                        assert np.array_equal(s1.download().reshape(F, m), got[b * F:(b + 1) * F]), what
                    f = 3 * F - 1                                        # a field alone: the bits it gives inside the batch
                    ctx.zone_restrict(x.ptr + 8 * f * n, 1, sf, apply_mass=mass)
                    assert np.array_equal(sf.download(), got[f]), what
                    ctx.zone_restrict(x, 3 * F, twice, apply_mass=mass)  # again: the same bits
                    assert np.array_equal(twice.download().reshape(3 * F, m), got), what
                    # Ginv = NULL scatters s itself
                    ctx.zone_prolong(s3, 3 * F, out)
                    plain = out.download().reshape(3 * F, n)
                    assert np.array_equal(plain, ref.scatter(got)), what
                    check_prolonged(plain, ref, what)
                    # the product, fed the device's s
                    ctx.zone_prolong(s3, 3 * F, out, Ginv=gd)
                    full = out.download().reshape(3 * F, n)
                    dref, db = ref.coeff(got, Ginv)
                    within(full, ref.scatter(dref), ref.scatter(db), what)
                    check_prolonged(full, ref, what)
                    ctx.zone_prolong(s3.ptr + 8 * f * m, 1, o1, Ginv=gd)         # one field alone: the same bits
                    assert np.array_equal(o1.download(), full[f]), what
                # prolong into the buffer the restrict read
                ctx.zone_restrict(x, 3 * F, s3, apply_mass=True)
                ctx.zone_prolong(s3, 3 * F, out, Ginv=gd)
                ctx.zone_prolong(s3, 3 * F, x, Ginv=gd)
                assert np.array_equal(x.download(), out.download()), (name, F, wide)
                for a in (x, s3, s1, sf, out, o1, twice):
                    a.free()
    finally:
        ctx.close()


PROJ_CASES = [(5, 0, "quadrants"), (5, 1, "mod3"), (5, 1, "each"), (21, 0, "quadrants"), (21, 1, "quadrants"), (21, 0, "mod3"),
              (21, 1, "one"), (46, 0, "split")]


@pytest.mark.parametrize("N,order,name", PROJ_CASES, ids=[f"n{N * N}-{'fenics' if o else 'vertex'}-{nm}" for N, o, nm in PROJ_CASES])
def test_projection_properties(hp, N, order, name):
    """G from the device against the dense chi^T M chi; P z = z for a zone-constant z, P(Px) = Px and chi^T M (x - Px) = 0,
    each to the bound of the module docstring (per zone j, with |Ginv| the entrywise magnitudes):
        |delta - a|_j <= (|Ginv| b_s)_j + b_delta_j + eps_P max|a|         for s = chi^T M chi a, delta = Ginv s
        |chi^T M (x - Px)|_j <= b_s(x - Px)_j + u (chi^T |M| (|x| + |Px|))_j + (|G| (|Ginv| b_s(x) + b_delta))_j + eps_P max|s|"""
    cs = cc.sb_case(N)
    n = cs["n"]
    lab_dof, m = extra_layout(N, name)
    lab = labels_dev(cs, lab_dof, order)
    rng = np.random.default_rng(7 * N + order)
    ctx = hp.Context(0)
    try:
        ctx.set_mesh_square(-1, 1, N - 1, order)
        ref = Ref(lab, m, mass_coo(ctx))
        ctx.set_control_zones(lab, m)
        chi = ref.scatter(np.eye(m))
        xd, g = ctx.array(chi), ctx.zeros(m * m)
        ctx.zone_restrict(xd, m, g, apply_mass=True)
        G = g.download().reshape(m, m)
        Gref = ref.restrict(chi, True)[0]
        eps_G = (ref.sizes.max() + W + 1) * U
        assert np.all(np.abs(G.astype(LD) - Gref) <= eps_G * np.abs(Gref)), name
        assert np.max(np.abs(G - czo.gram(lab_dof, m, cs["M"]))) <= 4 * eps_G * np.max(np.abs(G))
        G = 0.5 * (G + G.T)
        Ginv = np.linalg.inv(G)
        eps_P = np.linalg.norm(G, np.inf) * np.linalg.norm(Ginv, np.inf) * (eps_G + 8 * m * U)
        gi = ctx.array(Ginv)
        F = 5
        s, out, out2 = ctx.zeros(F * m), ctx.zeros(F * n), ctx.zeros(F * n)

        def project(host):
            """(P x, s, b_s, b_delta) of the device for the fields ``host``"""
            x = ctx.array(host)
            ctx.zone_restrict(x, F, s, apply_mass=True)
            ctx.zone_prolong(s, F, out, Ginv=gi)
            x.free()
            sd = s.download().reshape(F, m)
            return out.download().reshape(F, n), sd, ref.restrict(host, True)[1], ref.coeff(sd, Ginv)[1]

        aG, aGi = np.abs(G), np.abs(Ginv)
        # a zone-constant input comes back
        a = rng.standard_normal((F, m)) * 10.0 ** rng.uniform(-3, 3, (F, 1))
        z = ref.scatter(a)
        Pz, _, bs, bd = project(z)
        lim = bs @ aGi.T + bd + eps_P * np.abs(a).max(axis=1, keepdims=True)
        assert np.all(np.abs(Pz - z) <= ref.scatter(lim)), (name, float(np.max(np.abs(Pz - z) / np.maximum(ref.scatter(lim), 1e-300))))
        check_prolonged(Pz, ref, name)
        # P(Px) against Px, and the residual of x
        xh = rng.standard_normal((F, n))
        Px, sx, bsx, bdx = project(xh)
        ax = Px[:, [int(np.argmax(lab == j)) for j in range(m)]]
        PPx, _, bs2, bd2 = project(Px)
        lim = bs2 @ aGi.T + bd2 + eps_P * np.abs(ax).max(axis=1, keepdims=True)
        assert np.all(np.abs(PPx - Px) <= ref.scatter(lim)), name
        resid = xh - Px
        rd, r = ctx.array(resid), ctx.zeros(F * m)
        ctx.zone_restrict(rd, F, r, apply_mass=True)
        got = r.download().reshape(F, m)
        lim = (ref.restrict(resid, True)[1] + U * ref.zone_sum(ref.rows_of(np.abs(xh) + np.abs(Px))[1]).astype(np.float64)
               + (bsx @ aGi.T + bdx) @ aG.T + eps_P * np.abs(sx).max(axis=1, keepdims=True))
        assert np.all(np.abs(got) <= lim), (name, float(np.max(np.abs(got) / lim)))
    finally:
        ctx.close()


def test_bad_tables_raise_and_the_context_works_afterwards(hp):
    N = 5
    n = N * N
    ctx = hp.Context(0)
    try:
        with pytest.raises(ValueError):
            ctx.set_control_zones(np.zeros(n, dtype=np.int32), 1)          # before the mesh
        ctx.set_mesh_square(-1, 1, N - 1)
        x, s = ctx.array(np.arange(1.0, 2 * n + 1)), ctx.zeros(2 * n)
        for call in (lambda: ctx.zone_restrict(x, 1, s), lambda: ctx.zone_prolong(s, 1, x)):
            with pytest.raises(ValueError, match="control zones not set"):
                call()
        good = np.arange(n) % 3
        ctx.set_control_zones(good)
        ctx.zone_restrict(x, 2, s)
        before = s.download()[:6].copy()
        for bad, m in ((np.arange(n) % 3, 257), (np.arange(n) % 3, 0), (np.where(good == 1, 2, good), 3), (np.arange(n) % 4, 3),
                       (np.where(good == 0, -2, good), 3), (np.full(n, -1), 1)):
            with pytest.raises(ValueError):
                ctx.set_control_zones(bad, m)
        with pytest.raises(ValueError):
            ctx.set_control_zones(good[:-1])
        with pytest.raises(ValueError):
            ctx.zone_restrict(x, 0, s)
        with pytest.raises(ValueError):
            ctx.zone_restrict(None, 1, s)
        with pytest.raises(ValueError):
            ctx.zone_prolong(s, 1, None)
        ctx.zone_restrict(x, 2, s)                       # the previous table is still in place
        assert np.array_equal(s.download()[:6], before)
        assert np.array_equal(before[:3], [np.arange(1.0, n + 1)[good == j].sum() for j in range(3)])
        ctx.set_control_zones(None)
        with pytest.raises(ValueError, match="control zones not set"):
            ctx.zone_restrict(x, 1, s)
        ctx.set_control_zones(np.zeros(n, dtype=np.int64))
        ctx.zone_restrict(x, 1, s)
        assert s.download()[0] == n * (n + 1) / 2
        ctx.set_mesh_square(-1, 1, N)                    # a new mesh drops the table
        with pytest.raises(ValueError, match="control zones not set"):
            ctx.zone_restrict(x, 1, s)
        ctx.synchronize()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 2. the directions
def new_prob(hp, solvers, N, order):
    return solvers.SolidBodyDrift(hp.SquareMeshP1(-1, 1, N - 1), cc.NT, cc.sb_case(N)["dt"], om=cc.OM, order=order)


def zone_bound(ref, fields, mass, G, Ginv):
    """(reference, bound) of chi Ginv chi^T (M) x for the device's input ``fields``, per node: the three kernel terms with
    the device's own Ginv, plus eps_P max|delta| for the distance of that Ginv from the exact inverse (module docstring)"""
    s, bs = ref.restrict(fields, mass)
    d, bd = ref.coeff(s.astype(np.float64), Ginv)
    eps_G = (ref.sizes.max() + W + 1) * U
    eps_P = np.linalg.norm(G, np.inf) * np.linalg.norm(Ginv, np.inf) * (eps_G + 8 * ref.m * U)
    lim = bs @ np.abs(Ginv).T + bd + eps_P * np.abs(d).max(axis=1, keepdims=True).astype(np.float64)
    # the device rounds s to double before the product: one more u on every term of it
    lim = lim + U * (np.abs(s).astype(np.float64) @ np.abs(Ginv).T)
    return ref.scatter(d), ref.scatter(lim)


DIR_CASES = [("quadrants", None, False), ("quadrants", zc.IVL, False), ("mod3", None, True), ("mod3", zc.IVL, False)]


@pytest.mark.parametrize("order", [0, 1], ids=["vertex", "fenics"])
@pytest.mark.parametrize("name,ivl,smooth", DIR_CASES)
def test_solidbody_direction(hp, solvers, name, ivl, smooth, order):
    """d = chi G^-1 chi^T rhs at N = 21: componentwise against the extended-precision zone operation applied to the
    device's own right-hand side (left in ``scratch``; time-restricted by the device where intervals are given) to the
    bound of ``zone_bound``, and against the CPU oracle's direction to 1e-8, the loops' bar for the control."""
    N = 21
    cs = cc.sb_case(N)
    n, tl, Nt = cs["n"], cs["tl"], cc.NT
    lab_dof, m = zc.layout(N, name)
    lab = labels_dev(cs, lab_dof, order)
    zones = solvers.ControlZones(lab)
    ct = None if ivl is None else solvers.ControlIntervals(Nt, cc.INTERVALS[ivl])
    sm = solvers.Smoothness(2e-4, 4e-7) if smooth else None
    rng = np.random.default_rng(11)
    ck, pk = 1.0 + rng.random(tl), 0.05 * rng.standard_normal(tl)
    uk = np.tile(cs["u0"], Nt + 1) + 0.1 * rng.random(tl)
    prob = new_prob(hp, solvers, N, order)
    try:
        ctx = prob.ctx
        c, u, p = (ctx.array(to_dev(cs, a, order)) for a in (ck, uk, pk))
        d, rhs = ctx.zeros(tl), ctx.zeros(tl)
        kw = {} if sm is None else dict(smoothness=sm)
        if ct is not None:
            kw["control_time"] = ct
        prob.descent_direction(c, u, p, cc.BETA, d, scratch=rhs, control_space=zones, **kw)
        got = d.download().reshape(Nt + 1, n)
        _, _, G = prob._zones_cache[id(zones)]
        Ginv = prob.zones_device(zones).download().reshape(m, m)
        fields = rhs.download()
        if ct is not None:
            rk = ctx.zeros(ct.K * n)
            ctx.time_restrict(rhs, ct.starts, Nt, rk)
            fields = rk.download()
        ref = Ref(lab, m, mass_coo(ctx))
        dref, lim = zone_bound(ref, fields.reshape(-1, n), False, G, Ginv)
        if ct is not None:
            dref, lim = (np.repeat(a, np.diff(ct.starts), axis=0) for a in (dref, lim))
        within(got, dref, lim, (name, ivl, smooth))
        check_prolonged(got, ref, name)
        if ct is not None:
            assert ct.contains(got.ravel(), n)
        extra = None
        if smooth:
            import smoothness_oracle as smo
            extra = smo.smooth_rhs(cs["M"], cs["sb"].cm.Ad, ck, Nt, cs["dt"], sm.beta_x, sm.beta_t)
        d_o = czo.solidbody_direction(cs["sb"], ck, uk, pk, cc.BETA, n, Nt, lab_dof, m, None if ct is None else cc.INTERVALS[ivl],
                                      extra_rhs=extra)
        assert rel(to_dof(cs, got.ravel(), order), d_o) < 1e-8
    finally:
        prob.close()


@pytest.mark.parametrize("ivl,smooth", [(None, False), (zc.IVL, False), (None, True)])
def test_source_direction(hp, solvers, ivl, smooth):
    """d = P d_free on the solid-body mesh at N = 21 (quadrants, vertex order): componentwise against the extended-precision
    projection of the device's own free direction (time-restricted by the device where intervals are given)."""
    N, order, name = 21, 0, "quadrants"
    cs = cc.sb_case(N)
    n, tl, Nt = cs["n"], cs["tl"], cc.NT
    lab_dof, m = zc.layout(N, name)
    lab = labels_dev(cs, lab_dof, order)
    zones = solvers.ControlZones(lab)
    ct = None if ivl is None else solvers.ControlIntervals(Nt, cc.INTERVALS[ivl])
    kw = dict(smoothness=solvers.Smoothness(2e-4, 4e-7)) if smooth else {}
    rng = np.random.default_rng(12)
    prob = solvers.LinearSourceControl(hp.SquareMeshP1(-1, 1, N - 1), Nt, cs["dt"], solvers.rotation_wind(cc.OM), order=order)
    try:
        ctx = prob.ctx
        c, p = ctx.array(rng.random(tl)), ctx.array(0.1 * rng.standard_normal(tl))
        d, free = ctx.zeros(tl), ctx.zeros(tl)
        prob.descent_direction(c, p, 0.1, free, **kw)
        if ct is not None:
            kw["control_time"] = ct
        prob.descent_direction(c, p, 0.1, d, control_space=zones, **kw)
        got = d.download().reshape(Nt + 1, n)
        _, _, G = prob._zones_cache[id(zones)]
        Ginv = prob.zones_device(zones).download().reshape(m, m)
        fields = free.download()
        if ct is not None:
            rk = ctx.zeros(ct.K * n)
            ctx.time_restrict(free, ct.starts, Nt, rk)
            fields = rk.download()
        ref = Ref(lab, m, mass_coo(ctx))
        dref, lim = zone_bound(ref, fields.reshape(-1, n), True, G, Ginv)
        if ct is not None:
            dref, lim = (np.repeat(a, np.diff(ct.starts), axis=0) for a in (dref, lim))
        within(got, dref, lim, (ivl, smooth))
        check_prolonged(got, ref, name)
        d_o = czo.in_time(lambda x: czo.project(x, lab_dof, m, cs["M"]), to_dof(cs, free.download(), order),
                          None if ct is None else cc.INTERVALS[ivl], Nt, n)
        assert rel(to_dof(cs, got.ravel(), order), d_o) < 1e-8
    finally:
        prob.close()


def test_zones_device_caches_and_reregisters(hp, solvers):
    N, order = 5, 1
    cs = cc.sb_case(N)
    za, zb = solvers.ControlZones(zc.layout(N, "quadrants")[0]), solvers.ControlZones(zc.layout(N, "mod3")[0])
    prob = new_prob(hp, solvers, N, order)
    try:
        ga = prob.zones_device(za)
        assert prob.zones_device(za) is ga
        Ga = prob._zones_cache[id(za)][2]
        Go = czo.gram(za.labels, za.m, cs["M"])
        assert np.all(np.abs(Ga - Go) <= 4 * (za.sizes.max() + W + 1) * U * np.abs(Go)) and np.array_equal(Ga, Ga.T)
        gb = prob.zones_device(zb)
        assert gb is not ga and gb.count == 9 and ga.count == 16
        x, s = prob.ctx.array(np.ones(cs["n"])), prob.ctx.zeros(4)
        prob.ctx.zone_restrict(x, 1, s)
        assert list(s.download()[:3]) == list(zb.sizes)                 # zb's table is the registered one
        assert prob.zones_device(za) is ga                              # cached, and registered again
        prob.ctx.zone_restrict(x, 1, s)
        assert list(s.download()) == list(za.sizes)
        with pytest.raises(ValueError):
            prob.zones_device(solvers.ControlZones.single(cs["n"] + 1))
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 3. the loops
def check_against_oracle(cs, order, res, ref):
    """test_gpu_control_intervals.py's bars: armijo_k equal, costs rtol 1e-9, margins allclose(1e-6, 1e-9), c and u 1e-8"""
    u, _, c, h = res
    u_o, c_o, h_o = ref
    assert h["armijo_k"] == h_o["armijo_k"]
    assert np.allclose(h["cost"], h_o["cost"], rtol=1e-9, atol=0)
    for ms_d, ms_o in zip(h["armijo_margin"], h_o["armijo_margin"]):
        assert np.allclose(ms_d, ms_o, rtol=1e-6, atol=1e-9)
    assert rel(to_dof(cs, c, order), c_o) < 1e-8 and rel(to_dof(cs, u, order), u_o) < 1e-8


def check_subspace(zones, c, n, c_start=1.0):
    assert zones.contains(c, n)
    assert np.all(c.reshape(-1, n)[:, ~zones.active] == c_start)          # the inactive nodes hold c0 exactly


def zones_of(solvers, cs, N, name, order):
    return solvers.ControlZones(labels_dev(cs, zc.layout(N, name)[0], order))


def single_run(hp, solvers, N, order, optim, zones, ct, speculative=True, c_lower=cc.LO, fn=None, **kw):
    cs = cc.sb_case(N)
    prob = new_prob(hp, solvers, N, order)
    try:
        if fn is not None:
            return fn(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs[optim], order), np.ones(cs["tl"]), cc.BETA, c_lower,
                      cc.HI, cc.ITERS_SB, cc.GAM, cc.S0, cc.K_SB, control_space=zones, **kw)
        return solvers.pgd_solidbody(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs[optim], order), np.ones(cs["tl"]),
                                     cc.BETA, c_lower, cc.HI, cc.ITERS_SB, cc.GAM, cc.S0, cc.K_SB, speculative, None,
                                     optim=optim, control_time=ct, control_space=zones, **kw)
    finally:
        prob.close()


@pytest.mark.parametrize("speculative", [True, False], ids=["speculative", "sequential"])
@pytest.mark.parametrize("order", [0, 1], ids=["vertex", "fenics"])
@pytest.mark.parametrize("N,name,optim,ivl", zc.SB_CASES)
def test_pgd_solidbody_vs_cpu_loop(hp, solvers, N, name, optim, ivl, order, speculative):
    cs = cc.sb_case(N)
    zones = zones_of(solvers, cs, N, name, order)
    ct = None if ivl is None else solvers.ControlIntervals(cc.NT, cc.INTERVALS[ivl])
    ref = zc.sb_oracle(N, name, optim, ivl)
    assert ref[2]["armijo_margin_min"] >= zc.MARGIN_BAR
    res = single_run(hp, solvers, N, order, optim, zones, ct, speculative)
    check_against_oracle(cs, order, res, ref)
    check_subspace(zones, res[2], cs["n"])
    assert ct is None or ct.contains(res[2], cs["n"])
    assert zones.compact(res[2], cs["n"]).shape == (cc.NT + 1, zones.m)


def test_named_wrappers_pass_control_space_through(hp, solvers):
    N, order, name = 5, 1, "quadrants"
    cs = cc.sb_case(N)
    zones = zones_of(solvers, cs, N, name, order)
    for optim, fn in (("alltime", solvers.pgd_solidbody_alltime), ("finaltime", solvers.pgd_solidbody_finaltime)):
        res = single_run(hp, solvers, N, order, optim, zones, None, fn=fn)
        check_against_oracle(cs, order, res, zc.sb_oracle(N, name, optim, None))
        check_subspace(zones, res[2], cs["n"])


def test_pgd_solidbody_active_bound(hp, solvers):
    """c_lower = 0.62: the control reaches the bound in the third iteration (smallest margin 4.6e-2)"""
    N, name, optim, ivl = zc.ACTIVE_CASE
    order = 0
    cs = cc.sb_case(N)
    zones = zones_of(solvers, cs, N, name, order)
    ref = zc.sb_oracle(N, name, optim, ivl, zc.LO_ACTIVE)
    assert ref[2]["armijo_margin_min"] >= zc.MARGIN_BAR
    res = single_run(hp, solvers, N, order, optim, zones, None, c_lower=zc.LO_ACTIVE)
    check_against_oracle(cs, order, res, ref)
    check_subspace(zones, res[2], cs["n"])
    assert res[2].min() == zc.LO_ACTIVE


def test_pgd_solidbody_snapshots(hp, solvers):
    N, order = 21, 0
    cs = cc.sb_case(N)
    obs, u_o, c_o, h_o = zc.snap_oracle(solvers.Observations)
    assert h_o["armijo_margin_min"] >= zc.MARGIN_BAR
    zones = zones_of(solvers, cs, N, "quadrants", order)
    obs_dev = solvers.Observations(cc.NT, obs.levels, window=to_dev(cs, obs.window, order))
    prob = new_prob(hp, solvers, N, order)
    try:
        res = solvers.pgd_solidbody_snapshots(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs["alltime"], order), obs_dev,
                                              np.ones(cs["tl"]), cc.BETA, cc.LO, cc.HI, cc.ITERS_SB, cc.GAM, cc.S0_SNAP,
                                              cc.K_SB, control_space=zones)
    finally:
        prob.close()
    check_against_oracle(cs, order, res, (u_o, c_o, h_o))
    check_subspace(zones, res[2], cs["n"])


def test_lbfgs_solidbody(hp, solvers):
    L = zc.LBFGS_SB
    N, order = L["N"], 0
    cs = cc.sb_case(N)
    u_o, c_o, h_o = zc.lbfgs_sb_oracle()
    assert h_o["armijo_margin_min"] >= zc.MARGIN_BAR
    zones = zones_of(solvers, cs, N, L["name"], order)
    prob = new_prob(hp, solvers, N, order)
    try:
        res = solvers.lbfgs_solidbody(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs[L["optim"]], order), np.ones(cs["tl"]),
                                      cc.BETA, cc.LO, cc.HI, L["iters"], memory=L["memory"], gam=cc.GAM, s0=cc.S0,
                                      max_armijo=cc.K_SB, optim=L["optim"], control_space=zones)
    finally:
        prob.close()
    check_against_oracle(cs, order, res, (u_o, c_o, h_o))
    assert res[3]["used"] == h_o["used"]
    check_subspace(zones, res[2], cs["n"])


def source_prob(hp, solvers, pr):
    S = zc.SRC
    return solvers.LinearReactionSourceControl(hp.SquareMeshP1(0.0, 1.0, S["nc"]), pr["Nt"], pr["dt"], pr["wind"],
                                               pr["F"]["g"], eps=S["eps"], adjoint_mass=pr["sigma"])


def check_source(res, ref, zones, n):
    """test_gpu_control_intervals.py's bars for the source loops: the decisions of the CPU loop, costs to 1e-10, controls
    to 1e-9, state and adjoint to 1e-8, margins to 1e-8 absolute"""
    (ug, pg, cg, hg), (uo, po, co, ho) = res, ref
    assert ho["armijo_margin_min"] >= zc.MARGIN_BAR
    assert hg["armijo_k"] == ho["armijo_k"]
    keys = [k for k in ("cost", "cost_state") if k in ho]
    assert max(abs(a - b) / abs(b) for key in keys for a, b in zip(hg[key], ho[key])) <= 1e-10
    assert rel(cg, co) <= 1e-9 and rel(ug, uo) <= 1e-8 and rel(pg, po) <= 1e-8
    assert [len(m) for m in hg["armijo_margin"]] == [len(m) for m in ho["armijo_margin"]]
    assert max(abs(a - b) for mg, mo in zip(hg["armijo_margin"], ho["armijo_margin"]) for a, b in zip(mg, mo)) <= 1e-8
    check_subspace(zones, cg, n, 0.0)


@pytest.mark.parametrize("increment", ["linear", "resolve"])
def test_pgd_source_control_blocks(hp, solvers, increment):
    pr, lab, ref = zc.src_oracle(solvers.finaltime_exact_fields, solvers.finaltime_exact_wind(), increment)
    S, n, Nt = zc.SRC, pr["n"], pr["Nt"]
    zones = solvers.ControlZones.blocks(hp.SquareMeshP1(0.0, 1.0, S["nc"]), 2, 2)
    assert np.array_equal(zones.labels, lab)
    prob = source_prob(hp, solvers, pr)
    try:
        res = solvers.pgd_source_control(prob, pr["u0"], pr["uhat_T"], np.zeros((Nt + 1) * n), S["beta"], S["lo"], S["hi"],
                                         g=pr["F"]["f"], optim="finaltime", increment=increment, max_iters=S["iters"], tol=0.0,
                                         stop="cost", control_space=zones)
    finally:
        prob.close()
    assert res[3]["iterations"] == S["iters"]
    check_source(res, ref, zones, n)


def test_lbfgs_source_control_blocks(hp, solvers):
    pr, lab, ref = zc.lbfgs_src_oracle(solvers.finaltime_exact_fields, solvers.finaltime_exact_wind())
    S, n, Nt = zc.SRC, pr["n"], pr["Nt"]
    zones = solvers.ControlZones(lab)
    prob = source_prob(hp, solvers, pr)
    try:
        res = solvers.lbfgs_source_control(prob, pr["u0"], pr["uhat_T"], np.zeros((Nt + 1) * n), S["beta"], S["lo"], S["hi"],
                                           g=pr["F"]["f"], optim="finaltime", memory=5, max_iters=S["iters"], tol=0.0,
                                           stop="cost", control_space=zones)
    finally:
        prob.close()
    assert res[3]["used"] == ref[3]["used"] and len(res[3]["cost"]) == S["iters"]
    check_source(res, ref, zones, n)


def test_control_space_none_is_the_call_without_the_argument(hp, solvers):
    """fresh contexts (the sweep controller's budgets depend on a context's history): bitwise the same results"""
    N, order = 5, 0
    cs = cc.sb_case(N)
    runs = []
    for kw in ({}, dict(control_space=None)):
        prob = new_prob(hp, solvers, N, order)
        try:
            runs.append(solvers.pgd_solidbody(prob, to_dev(cs, cs["u0"], order), to_dev(cs, cs["alltime"], order),
                                              np.ones(cs["tl"]), cc.BETA, cc.LO, cc.HI, 2, cc.GAM, cc.S0, cc.K_SB,
                                              optim="alltime", **kw))
        finally:
            prob.close()
    (u0, p0, c0, h0), (u1, p1, c1, h1) = runs
    assert np.array_equal(u0, u1) and np.array_equal(p0, p1) and np.array_equal(c0, c1) and h0["cost"] == h1["cost"]
    pr, _, _ = zc.src_oracle(solvers.finaltime_exact_fields, solvers.finaltime_exact_wind(), "linear")
    S, n, Nt = zc.SRC, pr["n"], pr["Nt"]
    runs = []
    for kw in ({}, dict(control_space=None)):
        prob = source_prob(hp, solvers, pr)
        try:
            runs.append(solvers.pgd_source_control(prob, pr["u0"], pr["uhat_T"], np.zeros((Nt + 1) * n), S["beta"], S["lo"],
                                                   S["hi"], g=pr["F"]["f"], optim="finaltime", max_iters=2, tol=0.0,
                                                   stop="cost", **kw))
        finally:
            prob.close()
    (u0, p0, c0, h0), (u1, p1, c1, h1) = runs
    assert np.array_equal(u0, u1) and np.array_equal(p0, p1) and np.array_equal(c0, c1) and h0["cost"] == h1["cost"]


def test_start_control_outside_the_subspace_raises(hp, solvers):
    N, order = 5, 1
    cs = cc.sb_case(N)
    zones = zones_of(solvers, cs, N, "quadrants", order)
    c_bad = np.ones(cs["tl"])
    c_bad[cs["n"] + int(np.flatnonzero(zones.labels == 2)[1])] = 1.5
    prob = new_prob(hp, solvers, N, order)
    try:
        args = (cs["u0"], cs["alltime"])
        tail = (cc.BETA, cc.LO, cc.HI, 1, cc.GAM, cc.S0, 2)
        with pytest.raises(ValueError, match="not constant on the control zones"):
            solvers.pgd_solidbody(prob, *args, c_bad, *tail, optim="alltime", control_space=zones)
        with pytest.raises(ValueError, match="not constant on the control zones"):
            solvers.lbfgs_solidbody(prob, *args, c_bad, cc.BETA, cc.LO, cc.HI, 1, optim="alltime", control_space=zones)
        with pytest.raises(ValueError):
            solvers.pgd_solidbody(prob, *args, np.ones(cs["tl"]), *tail, optim="alltime",
                                  control_space=solvers.ControlZones.single(cs["n"] + 1))
        c_ok = zones.expand(np.arange(1.0, 5.0)[None, :] * np.ones((cc.NT + 1, 1)), base=0.25)
        u, _, c, _ = solvers.pgd_solidbody(prob, *args, c_ok, *tail, optim="alltime", control_space=zones)
        assert zones.contains(c, cs["n"]) and np.all(c.reshape(-1, cs["n"])[:, ~zones.active] == 0.25)
    finally:
        prob.close()


# ---------------------------------------------------------------------------------------------- 4. the example
def test_example_reduced_run_lowers_the_cost():
    ex = os.path.join(ROOT, "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "zone_control_pdeco.py"), "--reduced", "--iters", "3"],
                         capture_output=True, text=True, timeout=300, cwd=ex)
    assert out.returncode == 0, out.stderr[-2000:]
    costs = [float(ln.split("J =")[1].split()[0]) for ln in out.stdout.splitlines() if "J =" in ln]
    assert len(costs) == 3 and costs[-1] < costs[0]
    assert "constant on the zones: True, untouched elsewhere: True" in out.stdout
    assert "amplitudes" in out.stdout
