"""The mesh sizes of tests/test_gpu_mesh_sizes.py and their inputs (NumPy / SciPy only: checked by
tests/test_mesh_sizes_cases.py).

In vertex order every square mesh with 5 <= N <= 42 nodes per side runs its whole FEM-FCT step in k_mesh_step
(csrc/kernels_mesh.hip), whose control flow depends on N:

  * a thread owns a 2 x 2 block of nodes, TX = ceil(N / 2) blocks per side
  * the (TX - 2)^2 interior blocks go to the first waves, padded to whole waves of 64 (spare threads repeat block (1, 1));
    the 4 TX - 4 ring blocks go to the waves behind them (spare threads repeat block (0, 0))
  * for odd N the last block row and column hold nodes outside the mesh (loads redirected, stores to a trash word,
    operands zeroed)
  * ring blocks take per-node mass weights from triangle counts, interior blocks constants
  * N = 41 has instantiations of its own (N at compile time); every size comes with and without a non-flux matrix

SIZES lists the N at which one of these changes, each with its reason.  ``problem(N)`` are the inputs of a step there and
``node_classes(N)`` the nodes sorted by what the kernel does with them; the CPU test shows that the limiter cuts in every
class and that a subtly wrong scheme moves a node of every class by far more than the GPU test's bar.
"""
from collections import namedtuple

import numpy as np

import generic_patterns as gp

WAVE = 64
MEMBERS = 3
N_MIN, N_MAX = 5, 42                 # the sizes of the one-workgroup step with 2 x 2 blocks
THREADS = 512                        # its workgroup

Size = namedtuple("Size", "N TX reason")

SIZES = (
    Size(5, 3, "one interior block, 63 spare interior threads; odd"),
    Size(6, 3, "one interior block, 63 spare interior threads; even"),
    Size(7, 4, "four interior blocks; odd"),
    Size(8, 4, "four interior blocks; even"),
    Size(19, 10, "64 interior blocks: exactly one wave, no spare interior thread; odd"),
    Size(20, 10, "64 interior blocks: exactly one wave, no spare interior thread; even"),
    Size(33, 17, "64 ring blocks: exactly one wave of ring threads; odd"),
    Size(34, 17, "64 ring blocks: exactly one wave of ring threads; even"),
    Size(35, 18, "256 interior blocks: exactly four waves; odd"),
    Size(36, 18, "256 interior blocks: exactly four waves; even"),
    Size(39, 20, "the largest odd N on the run-time-N instantiations below 41"),
    Size(40, 20, "the largest even N on the run-time-N instantiations below 41"),
    Size(41, 21, "the compile-time-N instantiations, for one step against the oracle"),
    Size(42, 21, "the largest mesh that fits"),
)
BY_N = {s.N: s for s in SIZES}

# the step's variants: (rhs given, non-flux matrix given)
VARIANTS = {"no rhs, no N": (False, False), "rhs": (True, False), "rhs, N": (True, True)}

CLASSES = ("corner1", "corner2", "south", "north", "west", "east", "ring_inner", "deep")


def blocks_per_side(N, block=2):
    return -(-N // block)


def thread_layout(N):
    """what femfct_enqueue_mesh_step derives from N: interior blocks, the threads they take (whole waves), ring blocks,
    the ring's threads rounded up to whole waves"""
    TX = blocks_per_side(N)
    nint = (TX - 2) ** 2
    nint_pad = -(-nint // WAVE) * WAVE
    ring = 4 * TX - 4
    return dict(TX=TX, interior=nint, interior_threads=nint_pad, spare_interior=nint_pad - nint, ring=ring,
                ring_waves=-(-ring // WAVE), threads=nint_pad + ring)


def node_classes(N, block=2):
    """{class: node indices (vertex order, iy * N + ix)}, a partition of the N^2 nodes (block: nodes per side of a thread's
    block, 2 up to N = 42, 3 at N = 81):
         corner1      the corners in one triangle, (nc, 0) and (0, nc)
         corner2      the corners in two triangles, (0, 0) and (nc, nc)
         south, north, west, east
                      the sides without their corners (for odd N only north and east lie in partial blocks)
         ring_inner   interior nodes owned by a block of the block ring (ix // block or iy // block in {0, TX - 1})
         deep         interior nodes of interior blocks"""
    nc, TX = N - 1, blocks_per_side(N, block)
    iy, ix = np.divmod(np.arange(N * N), N)
    on_x, on_y = (ix == 0) | (ix == nc), (iy == 0) | (iy == nc)
    inner = ~on_x & ~on_y
    ring_block = np.isin(ix // block, (0, TX - 1)) | np.isin(iy // block, (0, TX - 1))
    masks = {
        "corner1": ((ix == nc) & (iy == 0)) | ((ix == 0) & (iy == nc)),
        "corner2": ((ix == 0) & (iy == 0)) | ((ix == nc) & (iy == nc)),
        "south": (iy == 0) & ~on_x, "north": (iy == nc) & ~on_x,
        "west": (ix == 0) & ~on_y, "east": (ix == nc) & ~on_y,
        "ring_inner": inner & ring_block, "deep": inner & ~ring_block,
    }
    return {k: np.flatnonzero(masks[k]) for k in CLASSES}


_PROBLEMS = {}


def matrices(N):
    return gp.square_mesh_matrices(N - 1)


def problem(N, B=MEMBERS):
    """B members on the N x N mesh of the unit square: own non-symmetric A (the rotation wind's, rescaled entry by entry
    for members 1 ..), own u_n and rhs, N = 0.05 M, one dt (gp.problem_of)"""
    if (N, B) not in _PROBLEMS:
        M, A = matrices(N)
        _PROBLEMS[(N, B)] = gp.problem_of(f"mesh_sizes{N}x{B}", M, [gp.rescaled(A, m) for m in range(B)])
    return _PROBLEMS[(N, B)]


def class_errors(N, err, block=2):
    """{class: worst entry of the per-node array ``err`` ([..., n]) over the class's nodes}"""
    err = np.asarray(err).reshape(-1, N * N)
    return {k: float(err[:, idx].max()) for k, idx in node_classes(N, block).items()}
