"""The hexagonal dependency cone of the lean tile sweeps (FEMFCT_TILE_CONE, FEMFCT_TILE_FIT), emulated in NumPy (no GPU).

The P1 stencil of the right-diagonal mesh has the six neighbours E, NE, N, W, SW, S: one step along (1, 1) costs one
sweep, one step along (1, -1) costs two, so K sweeps reach a hexagon and not the square that the max-norm distance
sweeps.  With ex, ey the signed excess of a patch node beyond the owned tile, its graph distance from the tile is
d = max(|ex|, |ey|) where ex ey >= 0 and |ex| + |ey| where not, and the rule is: live in sweep k iff k < min(kvalid,
K - d).  A workgroup's two-buffer lean loop under that rule (nodes that are not live write nothing; neighbours clamped
into the patch, as TileGeom::nb) is run here beside K sweeps of the whole mesh: the owned tile must hold the same bits.
The six (T, H, K, patch) cases are the launches of a flagship step, with the 32-patches and with the fitted 26- and
30-patches; the mesh sizes make the last patch end exactly on the mesh edge."""
import numpy as np
import pytest

DX = (1, 1, 0, -1, -1, 0)
DY = (0, 1, 1, 0, -1, -1)

# (T, H, K, PL, N, never live by the max-norm, never live by the hexagon): N = b T + T + H, so that the last patch
# ends on the mesh edge; the counts are those of a patch with no mesh edge near it
CASES = [
    (6, 13, 13, 32, 43, 124, 280),      # Jacobi, 13 sweeps
    (6, 13, 12, 32, 43, 240, 372),      # Jacobi, 12 sweeps
    (12, 10, 10, 32, 46, 124, 214),     # du/dt: r, then nine iterations
    (8, 12, 12, 32, 44, 124, 256),      # tail: ten iterations, fluxes, limiter
    (6, 10, 10, 26, 46, 100, 190),      # du/dt on the fitted patch
    (6, 12, 12, 30, 48, 116, 248),      # tail on the fitted patch
]
IDS = [f"T{c[0]}-H{c[1]}-K{c[2]}-P{c[3]}" for c in CASES]


def tile_geom(N, T, H, PL, bx, by):
    """TileGeom of kernels_tile32.hip for the PL x PL nodes of workgroup (bx, by), with both distances."""
    assert T + 2 * H == PL
    PLD = PL + 1
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
    ex = lx - np.clip(lx, H, H + T - 1)
    ey = ly - np.clip(ly, H, H + T - 1)
    dmax = np.maximum(np.abs(ex), np.abs(ey))
    dhex = np.where(ex * ey >= 0, dmax, np.abs(ex) + np.abs(ey))
    return dict(self=ly * PLD + lx, nb=nb, inside=inside, owned=owned, kvalid=kvalid, dmax=dmax, dhex=dhex, lx=lx, ly=ly,
                i=np.where(inside, gy * N + gx, 0), size=PL * PLD)


def mesh_rows(rng, N):
    """Rows of the whole mesh: about half of the off-diagonals exactly zero (upwind rows), a dominant diagonal; a slot
    whose neighbour lies outside the mesh is padding (coefficient 0, column = the row itself)."""
    i = np.arange(N * N)
    gx, gy = i % N, i // N
    off, col = np.zeros((6, N * N)), np.zeros((6, N * N), dtype=np.int64)
    for s in range(6):
        nx, ny = gx + DX[s], gy + DY[s]
        ex = (nx >= 0) & (nx < N) & (ny >= 0) & (ny < N)
        off[s] = -rng.random(N * N) * (rng.random(N * N) < 0.5) * ex
        col[s] = np.where(ex, ny * N + nx, i)
    dg = 1.0 + np.abs(off).sum(0) + rng.random(N * N)
    return off, col, dg, rng.standard_normal(N * N), rng.standard_normal(N * N)


def mesh_sweeps(off, col, dg, b, x, K):
    for _ in range(K):
        acc = b.copy()
        for s in range(6):
            acc = acc + (-off[s]) * x[col[s]]
        x = acc * (1.0 / dg)
    return x


def patch_sweeps_cone(g, off, dg, b, x, K):
    """The lean loop of one workgroup: two buffers that both start with the input, the node's own value in a register,
    a write only when live.  With the loads of the cone: the row where the node is ever live, the iterate where a live
    node can read it (d <= K); everything else is the zero of the kernel's defaults."""
    klive = np.minimum(g["kvalid"], K - g["dhex"])
    row = g["inside"] & (klive > 0)
    read = g["inside"] & (g["dhex"] <= K)
    lv = np.where(row, off[:, g["i"]], 0.0)
    dgp = np.where(row, dg[g["i"]], 1.0)
    bp = np.where(row, b[g["i"]], 0.0)
    xo = np.where(read, x[g["i"]], 0.0)
    bufs = np.zeros((2, g["size"]))
    bufs[0][g["self"]] = xo
    bufs[1][g["self"]] = xo
    for k in range(K):
        c, o = bufs[k & 1], bufs[(k + 1) & 1]
        live = k < klive
        acc = bp.copy()
        for s in range(6):
            acc = acc + (-lv[s]) * c[g["nb"][s]]
        xo = np.where(live, acc * (1.0 / dgp), xo)
        o[g["self"][live]] = xo[live]
    return xo


@pytest.mark.parametrize("T,H,K,PL,N,nmax,nhex", CASES, ids=IDS)
def test_cone_sweeps_keep_the_owned_bits(T, H, K, PL, N, nmax, nhex):
    """Every workgroup of a mesh whose last patch ends exactly on the mesh edge, against K sweeps of the whole mesh."""
    assert (N - T - H) % T == 0
    rng = np.random.default_rng(1000 * T + 10 * H + K)
    off, col, dg, b, x = mesh_rows(rng, N)
    ref = mesh_sweeps(off, col, dg, b, x, K)
    t = -(-N // T)
    on_edge = 0
    for by in range(t):
        for bx in range(t):
            g = tile_geom(N, T, H, PL, bx, by)
            on_edge += int(bx * T - H + PL - 1 == N - 1) + int(by * T - H + PL - 1 == N - 1)
            got = patch_sweeps_cone(g, off, dg, b, x, K)
            own = g["owned"]
            assert own.any()
            assert np.array_equal(got[own], ref[g["i"][own]]), (bx, by)
    assert on_edge >= 2 * t


@pytest.mark.parametrize("T,H,K,PL,N,nmax,nhex", CASES, ids=IDS)
def test_never_live_counts(T, H, K, PL, N, nmax, nhex):
    """Nodes of a patch away from the mesh edge that no sweep ever updates: their rows are not loaded."""
    g = tile_geom(50 * T + 1, T, H, PL, 20, 20)
    assert g["inside"].all()
    assert int((np.minimum(g["kvalid"], K - g["dmax"]) <= 0).sum()) == nmax
    assert int((np.minimum(g["kvalid"], K - g["dhex"]) <= 0).sum()) == nhex


@pytest.mark.parametrize("T,H,K,PL,N,nmax,nhex", CASES, ids=IDS)
def test_hex_distance_is_the_graph_distance_and_lipschitz(T, H, K, PL, N, nmax, nhex):
    """d is the number of stencil steps to the tile (breadth-first search over the six slots), it changes by at most
    one along every slot -- what the proof of the live rule uses -- and the branch-free form of the kernel agrees."""
    g = tile_geom(50 * T + 1, T, H, PL, 20, 20)
    lx, ly, d = g["lx"], g["ly"], g["dhex"].reshape(PL, PL)
    for s in range(6):
        nx, ny = lx + DX[s], ly + DY[s]
        ok = (nx >= 0) & (nx < PL) & (ny >= 0) & (ny < PL)
        assert (np.abs(d[ny[ok], nx[ok]] - d[ly[ok], lx[ok]]) <= 1).all()
    bfs = np.where(d == 0, 0, 1 << 20)
    for _ in range(2 * PL):
        new = bfs.copy()
        for s in range(6):
            sh = np.full_like(bfs, 1 << 20)
            ys, xs = slice(max(DY[s], 0), PL + min(DY[s], 0)), slice(max(DX[s], 0), PL + min(DX[s], 0))
            yd, xd = slice(max(-DY[s], 0), PL + min(-DY[s], 0)), slice(max(-DX[s], 0), PL + min(-DX[s], 0))
            sh[yd, xd] = bfs[ys, xs] + 1
            new = np.minimum(new, sh)
        bfs = new
    assert np.array_equal(bfs, d)
    ex = lx - np.clip(lx, H, H + T - 1)
    ey = ly - np.clip(ly, H, H + T - 1)
    assert np.array_equal(np.maximum(np.maximum(np.abs(ex), np.abs(ey)), np.abs(ex - ey)), g["dhex"])


def test_node_updates_fall_to_a_third():
    """H = K = 13: node updates of a launch, as a share of K x 1024, by the max-norm and by the hexagon."""
    g = tile_geom(301, 6, 13, 32, 20, 20)
    upd = lambda d: int(np.clip(np.minimum(g["kvalid"], 13 - d), 0, None).sum()) / (13 * 1024)
    assert 0.36 < upd(g["dmax"]) < 0.38
    assert 0.31 < upd(g["dhex"]) < 0.33
