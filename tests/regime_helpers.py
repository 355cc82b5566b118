"""What the GPU tests of the kernel regimes share: the tuning knobs that move a size class to other kernels, and a
generic (non-mesh) sparsity pattern."""
import os

from scipy.sparse import csr_matrix, lil_matrix

# tuning knobs that move a size class to other kernels (or the species solve to BiCGStab): the regime and Chebyshev
# assertions hold for their defaults; the oracle comparisons hold whatever they are set to
REGIME_KNOBS = ("FEMFCT_TILES", "FEMFCT_STRIPS", "FEMFCT_IMPLICIT", "FEMFCT_TILE4", "FEMFCT_T4_DPP", "FEMFCT_T4_K",
                "FEMFCT_T4_WALK", "FEMFCT_MESH_SOLVE", "FEMFCT_SINGLE_PATCH_BATCH", "FEMFCT_SPECIES_SOLVER",
                "FEMFCT_DEEP_HALO", "FEMFCT_WG_SLOTS", "FEMFCT_STRIP_K", "FEMFCT_MESH_STEP_BATCH_LARGE")


def regime_knobs_default():
    return not any(k in os.environ for k in REGIME_KNOBS)


def nine_point_problem(N, rng):
    """A 'mass' matrix and a flux matrix on the 9-point stencil graph of an N x N grid (ELL width 9,
    not a P1 mesh): exercises the runtime-width kernels and the strip-fused path on a generic pattern."""
    n = N * N
    M = lil_matrix((n, n))
    A = lil_matrix((n, n))
    for iy in range(N):
        for ix in range(N):
            i = iy * N + ix
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    jx, jy = ix + dx, iy + dy
                    if 0 <= jx < N and 0 <= jy < N:
                        j = jy * N + jx
                        M[i, j] = 4.0 if i == j else 0.25 + 0.1 * ((i + j) % 3)
                        A[i, j] = rng.standard_normal() * (1.0 if i != j else 0.3)
    M = csr_matrix(M)
    M = (M + M.T) * 0.5
    return csr_matrix(M), csr_matrix(A)
