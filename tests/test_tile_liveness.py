"""The liveness rule of the lean 32 x 32 tile sweeps (FEMFCT_TILE_LEAN), emulated in NumPy (no GPU).

A workgroup stages a 32 x 32 patch = tile + halo H and runs K sweeps; a node's value is exact for sweeps k < kvalid
(the halo shrinks by one ring per sweep).  The present loops update every node with k < kvalid and copy the others
forward; the lean loops update a node only while the owned tile can still see the result -- a node at max-norm distance
d from the tile through sweep K - 1 - d at the latest -- write only then, and ping-pong between two buffers that both
start with the input.  Both rules are run here on every tile of several meshes with the same arithmetic: what the
owned tile ends with must be the same bits."""
import numpy as np
import pytest

PL, PLD = 32, 33
DX = (1, 1, 0, -1, -1, 0)
DY = (0, 1, 1, 0, -1, -1)
CASES = [(81, 13, 13), (81, 13, 7), (81, 10, 10), (41, 12, 12), (33, 8, 8), (45, 13, 13), (43, 13, 13)]


def tile_geom(N, H, bx, by):
    """TileGeom of kernels_tile32.hip for all 1024 threads of workgroup (bx, by)."""
    T = PL - 2 * H
    tid = np.arange(PL * PL)
    lx, ly = tid % PL, tid // PL
    x0, y0 = bx * T - H, by * T - H
    gx, gy = x0 + lx, y0 + ly
    inside = (gx >= 0) & (gx < N) & (gy >= 0) & (gy < N)
    owned = inside & (lx >= H) & (lx < H + T) & (ly >= H) & (ly < H + T)
    kv = np.full(PL * PL, 1 << 20)
    if x0 > 0:
        kv = np.minimum(kv, lx)
    if x0 + PL - 1 < N - 1:
        kv = np.minimum(kv, PL - 1 - lx)
    if y0 > 0:
        kv = np.minimum(kv, ly)
    if y0 + PL - 1 < N - 1:
        kv = np.minimum(kv, PL - 1 - ly)
    kvalid = np.where(inside, kv, 0)
    nb = np.stack([np.clip(ly + DY[s], 0, PL - 1) * PLD + np.clip(lx + DX[s], 0, PL - 1) for s in range(6)])
    ddx = np.maximum(np.maximum(H - lx, lx - (H + T - 1)), 0)
    ddy = np.maximum(np.maximum(H - ly, ly - (H + T - 1)), 0)
    # a slot whose neighbour lies outside the mesh is padding: coefficient 0
    exists = np.stack([(gx + DX[s] >= 0) & (gx + DX[s] < N) & (gy + DY[s] >= 0) & (gy + DY[s] < N) & inside
                       for s in range(6)])
    return dict(self=ly * PLD + lx, nb=nb, inside=inside, owned=owned, kvalid=kvalid, d=np.maximum(ddx, ddy),
                exists=exists, wave=tid // 64)


def tiles(N, H):
    t = -(-N // (PL - 2 * H))
    return [(bx, by) for by in range(t) for bx in range(t)]


def random_rows(rng, g):
    """Rows with half the off-diagonals exactly zero (upwind rows), a dominant diagonal, zero outside the mesh."""
    off = -rng.random((6, PL * PL)) * (rng.random((6, PL * PL)) < 0.5) * g["exists"]
    dg = np.where(g["inside"], 1.0 + np.abs(off).sum(0) + rng.random(PL * PL), 1.0)
    b = np.where(g["inside"], rng.standard_normal(PL * PL), 0.0)
    x = np.where(g["inside"], rng.standard_normal(PL * PL), 0.0)
    return off, dg, b, x


def jacobi_present(g, off, dg, b, x, K):
    bufs = np.zeros((2, PL * PLD))
    bufs[0][g["self"]] = x
    cur, waves = 0, 0
    for k in range(K):
        c = bufs[cur]
        xn = c[g["self"]].copy()
        live = k < g["kvalid"]
        acc = b.copy()
        for s in range(6):
            acc = acc + (-off[s]) * c[g["nb"][s]]
        xn[live] = (acc * (1.0 / dg))[live]
        bufs[cur ^ 1][g["self"]] = xn
        cur ^= 1
        waves += 16                                  # every wave runs the sweep
    return bufs[cur][g["self"]], waves


def jacobi_lean(g, off, dg, b, x, K):
    bufs = np.zeros((2, PL * PLD))
    bufs[0][g["self"]] = x
    bufs[1][g["self"]] = x
    klive = np.minimum(g["kvalid"], K - g["d"])
    xo, waves = x.copy(), 0
    for k in range(K):
        c, o = bufs[k & 1], bufs[(k + 1) & 1]
        live = k < klive
        acc = b.copy()
        for s in range(6):
            acc = acc + (-off[s]) * c[g["nb"][s]]
        xo[live] = (acc * (1.0 / dg))[live]
        o[g["self"][live]] = xo[live]                # written only when live
        waves += len(np.unique(g["wave"][live]))     # waves with no live lane only reach the barrier
    return xo, waves


@pytest.mark.parametrize("N,H,K", CASES)
def test_jacobi_live_rule_keeps_the_owned_bits(N, H, K):
    rng = np.random.default_rng(N * 1000 + H * 10 + K)
    for bx, by in tiles(N, H):
        g = tile_geom(N, H, bx, by)
        rows = random_rows(rng, g)
        ref, _ = jacobi_present(g, *rows, K)
        got, _ = jacobi_lean(g, *rows, K)
        assert g["owned"].any()
        assert np.array_equal(ref[g["owned"]], got[g["owned"]]), (bx, by)


def test_live_rule_runs_under_six_tenths_of_the_wave_sweeps():
    """(81, 13, 13), the flagship's Jacobi launches: 22 400 of 40 768 wave-sweeps (0.549)."""
    N, H, K = 81, 13, 13
    rng = np.random.default_rng(7)
    present = lean = 0
    for bx, by in tiles(N, H):
        g = tile_geom(N, H, bx, by)
        rows = random_rows(rng, g)
        present += jacobi_present(g, *rows, K)[1]
        lean += jacobi_lean(g, *rows, K)[1]
    print(f"wave-sweeps: present {present}, live rule {lean}, ratio {lean / present:.3f}")
    assert present == 16 * K * len(tiles(N, H))
    assert lean < 0.6 * present


# ---- the three-term Chebyshev recurrence: y_new = w_k (z + y_mid - y_old) + y_old, z = (b - M y_mid) / (scale m_ii) ----

def mass_rows(rng, g):
    mv = (0.5 + rng.random((6, PL * PL))) * g["exists"]
    md = np.where(g["inside"], 4.0 + rng.random(PL * PL), 1.0)
    b = np.where(g["inside"], rng.standard_normal(PL * PL), 0.0)
    ym = np.where(g["inside"], rng.standard_normal(PL * PL), 0.0)
    yo = np.where(g["inside"], rng.standard_normal(PL * PL), 0.0)
    return mv, md, b, ym, yo


def cheb_present(g, mv, md, b, ym, yo, w, valid):
    """Three rotating buffers, every node written every iteration (copied forward when not valid(k))."""
    ys = np.zeros((3, PL * PLD))
    ys[0][g["self"]] = yo
    ys[1][g["self"]] = ym
    io, im, in_ = 0, 1, 2
    for k in range(len(w)):
        ymd = ys[im]
        ymv = ymd[g["self"]]
        acc = md * ymv
        for s in range(6):
            acc = acc + mv[s] * ymd[g["nb"][s]]
        z = (b - acc) * (1.0 / (1.5 * md))
        yov = ys[io][g["self"]]
        yn = np.where(valid(k), w[k] * (z + ymv - yov) + yov, ymv)
        ys[in_][g["self"]] = yn
        io, im, in_ = im, in_, io
    return ys[im], ys[io]


def cheb_lean(g, mv, md, b, ym, yo, w, live, first=0):
    """Two buffers of y_mid, both starting with the input; y_mid / y_old of the node itself in registers.
    `first`: the buffer iteration 0 reads."""
    ys = np.zeros((2, PL * PLD))
    ys[0][g["self"]] = ym
    ys[1][g["self"]] = ym
    ym, yo = ym.copy(), yo.copy()
    for k in range(len(w)):
        c, o = ys[(k + first) & 1], ys[(k + first + 1) & 1]
        lv = live(k)
        acc = md * ym
        for s in range(6):
            acc = acc + mv[s] * c[g["nb"][s]]
        z = (b - acc) * (1.0 / (1.5 * md))
        yn = w[k] * (z + ym - yo) + yo
        yo = np.where(lv, ym, yo)
        ym = np.where(lv, yn, ym)
        o[g["self"][lv]] = ym[lv]
    return ym, yo, ys[(len(w) + first) & 1]


@pytest.mark.parametrize("N,H,K", CASES)
def test_cheb_live_rule_keeps_the_owned_bits(N, H, K):
    """k_tile_cheb: update while k < min(kvalid, K - d); y_mid and y_old of the owned nodes."""
    rng = np.random.default_rng(N * 1000 + H * 10 + K + 1)
    w = 1.0 + rng.random(K)
    for bx, by in tiles(N, H):
        g = tile_geom(N, H, bx, by)
        rows = mass_rows(rng, g)
        mid, old = cheb_present(g, *rows, w, lambda k: k < g["kvalid"])
        ym, yo, _ = cheb_lean(g, *rows, w, lambda k: k < np.minimum(g["kvalid"], K - g["d"]))
        own = g["owned"]
        assert np.array_equal(mid[g["self"]][own], ym[own]), (bx, by)
        assert np.array_equal(old[g["self"]][own], yo[own]), (bx, by)


@pytest.mark.parametrize("N,H,K", CASES)
def test_dudt_cheb_live_rule_keeps_the_owned_bits(N, H, K):
    """k_tile_dudt_cheb: one ring is spent on r = rhs - A u_L, so iteration k needs k + 1 < kvalid; live while
    additionally k < K - d.  At most H - 1 iterations fit the halo."""
    K = min(K, H - 1)
    rng = np.random.default_rng(N * 1000 + H * 10 + K + 2)
    w = 1.0 + rng.random(K)
    for bx, by in tiles(N, H):
        g = tile_geom(N, H, bx, by)
        mv, md, _, u, _ = mass_rows(rng, g)
        av = rng.standard_normal((6, PL * PL)) * g["exists"]
        us = np.zeros(PL * PLD)
        us[g["self"]] = u
        acc = md * u
        for s in range(6):
            acc = acc + av[s] * us[g["nb"][s]]
        r = np.where(g["kvalid"] >= 1, -acc, 0.0)
        y1 = np.where(g["kvalid"] >= 1, 0.9 * (r / (1.5 * md)), 0.0)
        zero = np.zeros(PL * PL)
        mid, old = cheb_present(g, mv, md, r, y1, zero, w, lambda k: k + 1 < g["kvalid"])
        ym, yo, _ = cheb_lean(g, mv, md, r, y1, zero, w, lambda k: (k + 1 < g["kvalid"]) & (k < K - g["d"]), first=1)
        own = g["owned"]
        assert np.array_equal(mid[g["self"]][own], ym[own]), (bx, by)
        assert np.array_equal(old[g["self"]][own], yo[own]), (bx, by)


@pytest.mark.parametrize("N,H,K", CASES)
def test_cheb_flux_limit_live_rule_keeps_du_two_rings_out(N, H, K):
    """k_tile_cheb_flux_limit: the fluxes of the tile and its first ring read the final du of their six neighbours, so
    du is needed two rings out: live while k < min(kvalid, K - max(d - 2, 0)).  At most H - 2 iterations fit the halo.
    Compared: everything the flux phase reads -- du of every node within one ring of the tile whose neighbours all
    carry the final du (kvalid >= K + 1), from the register and from the last buffer, and du of its six neighbours
    from the last buffer."""
    K = min(K, H - 2)
    rng = np.random.default_rng(N * 1000 + H * 10 + K + 3)
    w = 1.0 + rng.random(K)
    for bx, by in tiles(N, H):
        g = tile_geom(N, H, bx, by)
        rows = mass_rows(rng, g)
        mid, _ = cheb_present(g, *rows, w, lambda k: k < g["kvalid"])
        ym, _, last = cheb_lean(g, *rows, w, lambda k: k < np.minimum(g["kvalid"], K - np.maximum(g["d"] - 2, 0)))
        have = g["inside"] & (g["kvalid"] >= K + 1) & (g["d"] <= 1)
        assert have[g["owned"]].all()
        assert np.array_equal(mid[g["self"]][have], ym[have]), (bx, by)
        assert np.array_equal(mid[g["self"]][have], last[g["self"]][have]), (bx, by)
        for s in range(6):
            assert np.array_equal(mid[g["nb"][s]][have], last[g["nb"][s]][have]), (bx, by, s)
