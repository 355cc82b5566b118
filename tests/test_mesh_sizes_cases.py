"""The sizes and the inputs of tests/test_gpu_mesh_sizes.py (tests/mesh_sizes_cases.py): no GPU needed.  The sizes are the
ones their reasons state, the node classes partition the mesh, and at every size the data makes the low-order solve
converge, the limiter cut in every node class, and a subtly wrong scheme show in every node class."""
import numpy as np
import pytest

import generic_patterns as gp
import mesh_sizes_cases as ms
from oracle import fct as ofct

SIZE_IDS = [f"N{s.N}" for s in ms.SIZES]
SPOIL_BAR = 1e-6                    # of max |ref|: three orders above the GPU test's per-node bar of 1e-9


def test_sizes_are_what_their_reasons_state():
    Ns = [s.N for s in ms.SIZES]
    assert Ns == [5, 6, 7, 8, 19, 20, 33, 34, 35, 36, 39, 40, 41, 42] and len(ms.BY_N) == len(Ns)
    assert ms.N_MIN == min(Ns) and ms.N_MAX == max(Ns)
    L = {s.N: ms.thread_layout(s.N) for s in ms.SIZES}
    for s in ms.SIZES:
        assert s.TX == L[s.N]["TX"] == -(-s.N // 2), s
        assert L[s.N]["threads"] <= ms.THREADS, s
        assert ("odd" in s.reason) == (s.N % 2 == 1) or s.N > 40, s
    for N in (5, 6):
        assert L[N]["interior"] == 1 and L[N]["spare_interior"] == 63
    for N in (7, 8):
        assert L[N]["interior"] == 4
    for N in (19, 20):
        assert L[N]["interior"] == 64 and L[N]["spare_interior"] == 0 and L[N]["interior_threads"] == 64
    for N in (33, 34):
        assert L[N]["ring"] == 64 and L[N]["ring_waves"] == 1
    assert ms.thread_layout(32)["ring"] < 64 < L[35]["ring"] and L[35]["ring_waves"] == 2
    for N in (35, 36):
        assert L[N]["interior"] == 256 and L[N]["spare_interior"] == 0
    assert all(ms.thread_layout(N)["spare_interior"] > 0 for N in range(5, 43) if N not in (19, 20, 35, 36))
    assert ms.thread_layout(42)["threads"] == 464 and ms.thread_layout(43)["TX"] == 22
    # both parities next to each other below the compile-time-N size, and that size itself
    assert {39, 40, 41, 42} <= set(Ns)


@pytest.mark.parametrize("size", ms.SIZES, ids=SIZE_IDS)
def test_node_classes_partition_the_mesh(size):
    N, nc, TX = size.N, size.N - 1, size.TX
    cls = ms.node_classes(N)
    assert tuple(cls) == ms.CLASSES
    allnodes = np.concatenate(list(cls.values()))
    assert np.array_equal(np.sort(allnodes), np.arange(N * N))
    assert all(idx.size > 0 for idx in cls.values())
    assert sorted(cls["corner1"].tolist()) == [nc, nc * N] and sorted(cls["corner2"].tolist()) == [0, N * N - 1]
    for side in ("south", "north", "west", "east"):
        assert cls[side].size == N - 2
    assert cls["deep"].size + cls["ring_inner"].size == (N - 2) ** 2
    # the classes are the mesh's: entries per row of the mass matrix (triangles + 1 at a corner, 5 on a side, 7 inside)
    M, _ = ms.matrices(N)
    row = np.diff(M.indptr)
    assert np.all(row[cls["corner1"]] == 3) and np.all(row[cls["corner2"]] == 4)
    for side in ("south", "north", "west", "east"):
        assert np.all(row[cls[side]] == 5)
    assert np.all(row[cls["ring_inner"]] == 7) and np.all(row[cls["deep"]] == 7)
    # deep nodes: the nodes of the (TX - 2)^2 interior blocks that lie inside the mesh and off its boundary
    iy, ix = np.divmod(cls["deep"], N)
    assert ix.min() == iy.min() == 2 and ix.max() == iy.max() == min(2 * (TX - 1) - 1, nc - 1)
    want = (min(2 * (TX - 1), nc) - 2) ** 2
    assert cls["deep"].size == want
    # for odd N the last block row and column are partial: their nodes inside the mesh are north, east and a corner each
    if N % 2:
        assert 2 * (TX - 1) == nc


@pytest.mark.parametrize("size", ms.SIZES, ids=SIZE_IDS)
def test_inputs_are_as_described(size):
    N = size.N
    P = ms.problem(N)
    assert P.n == N * N and len(P.A) == len(P.u_n) == len(P.rhs) == ms.MEMBERS and 0 < P.dt <= 1.0
    assert gp.width(P.M) == 7 and abs(P.N - 0.05 * P.M).max() < 1e-17
    for m in range(ms.MEMBERS):
        assert np.array_equal(P.A[m].indices, P.M.indices)
        assert abs(P.A[m] - P.A[m].T).max() > 1e-3 * abs(P.A[m]).max()          # not symmetric
        for k in range(m):
            assert not np.array_equal(P.A[m].data, P.A[k].data)
            assert not np.array_equal(P.u_n[m], P.u_n[k]) and not np.array_equal(P.rhs[m], P.rhs[k])
        for Nmat in (None, P.N):
            diag, _ = gp.low_order(P.M, P.A[m], P.ml, P.dt, Nmat)
            g = gp.jacobi_norm(P.M, P.A[m], P.ml, P.dt, Nmat)
            assert np.all(diag > 0) and g <= 0.5, (N, m, g)
    assert ms.problem(N, 1).A[0] is not None and np.array_equal(ms.problem(N, 1).u_n[0], P.u_n[0])


def _oracle(P, m, rhs, N):
    info = {}
    u = ofct.fct_step(P.A[m], P.rhs[m] if rhs else np.zeros(P.n), P.u_n[m], P.dt, P.n, P.M, P.ML, None,
                      non_flux_mat=P.N if N else None, info=info)
    return u, info


@pytest.mark.parametrize("size", ms.SIZES, ids=SIZE_IDS)
def test_limiter_cuts_and_spoilt_rules_show_in_every_node_class(size):
    """Per size: the restated step is the oracle's; the limiter cuts >= 25 % of the rows in every member and variant and
    some row of every node class in some member; every rule of gp.SPOILS moves some node of every class by more than
    1e-6 max |ref| in some member, without rhs and N and with both."""
    N = size.N
    P = ms.problem(N)
    cls = ms.node_classes(N)
    worst_cut, weakest = 1.0, np.inf
    for variant, (rhs, Nm) in ms.VARIANTS.items():
        cut_in = {k: False for k in cls}
        moved = {(s, k): 0.0 for s in gp.SPOILS for k in cls}
        for m in range(ms.MEMBERS):
            ref, info = _oracle(P, m, rhs, Nm)
            assert np.all(np.isfinite(ref))
            cut = (info["r_pos"] < 1) | (info["r_neg"] < 1)
            worst_cut = min(worst_cut, cut.mean())
            assert cut.mean() >= 0.25, (N, variant, m, cut.mean())
            for k, idx in cls.items():
                cut_in[k] |= bool(cut[idx].any())
            if rhs != Nm:
                continue                        # the power check: without rhs and N, and with both
            args = (P.A[m], P.rhs[m] if rhs else np.zeros(P.n), P.u_n[m], P.dt, P.M, P.ml, P.N if Nm else None)
            true = gp.spoilt_step(*args, spoil=None)
            assert np.linalg.norm(true - ref) <= 1e-14 * np.linalg.norm(ref), (N, variant, m)
            for s in gp.SPOILS:
                d = np.abs(gp.spoilt_step(*args, spoil=s) - ref) / np.abs(ref).max()
                for k, idx in cls.items():
                    moved[(s, k)] = max(moved[(s, k)], float(d[idx].max()))
        assert all(cut_in.values()), (N, variant, cut_in)
        if rhs == Nm:
            weakest = min(weakest, min(moved.values()))
            assert all(v > SPOIL_BAR for v in moved.values()), (N, variant, {k: v for k, v in moved.items() if v <= SPOIL_BAR})
    print(f"[mesh sizes] N={N}: dt={P.dt:.4f}, smallest cut fraction={worst_cut:.2f}, weakest spoil signal={weakest:.2e}")
