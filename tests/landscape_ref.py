"""Shared by tests/test_landscape_ref.py, tests/test_landscape_plan.py, tests/test_landscape_front.py (CPU) and
tests/test_gpu_landscape.py (GPU): a plain numpy / Python restatement of ``EnergyLandscape`` written from the definitions of
``DESIGN.md`` section 25 and not from the kernel, and the designed tetragonal host.

Voxel centre.  ``f_a = (i_a + 0.5) / n_a`` and ``x_k = (f0 cell[0][k] + f1 cell[1][k]) + f2 cell[2][k]``: numpy's IEEE operations in
this order.  Term.  That of ``tests/barrier_ref.py``: ``b = x - s``, ``T = (m0 cell[0] + m1 cell[1]) + m2 cell[2]``, ``d = b - T``,
``dd = (d0 d0 + d1 d1) + d2 d2``, counted where ``dd <= rc rc``, value ``phi(dd)``.  The triples are found by brute force over
``rint(crystal(b)) + t`` with ``|t_a| <= ceil(rc / h_a) + 1``: a term within ``rc`` has ``|crystal(b)_a - m_a| <= rc / h_a`` and
``|crystal(b)_a - rint(.)| <= 1 / 2``.  Sum.  The counted terms sorted by ``(s, m0, m1, m2)`` and added one after the other in a
Python loop, from 0.0.
"""
import itertools

import numpy as np

from tests import barrier_ref as BR

TILE = (4, 8, 8)
THREADS = 256
CHUNK = 448
MAX_GRID = 1024
MAX_VOXELS = 1 << 27


def fractional(i, n):
    return (np.asarray(i, dtype=np.float64) + 0.5) / np.float64(n)


def center(cell, grid, i):
    """The centre of voxel ``i = (i0, i1, i2)``."""
    cell = np.asarray(cell, dtype=np.float64)
    f = [fractional(i[a], grid[a]) for a in range(3)]
    return (f[0] * cell[0] + f[1] * cell[1]) + f[2] * cell[2]


def unflatten(grid, v):
    return (v // (grid[1] * grid[2]), v // grid[2] % grid[1], v % grid[2])


def voxel_terms(cell, static_pos, eps, sigma, rc, x, extra=1):
    """(phi, dd, atom, m) of the counted terms of a probe at ``x``, sorted by ``(atom, m0, m1, m2)``."""
    cell = np.asarray(cell, dtype=np.float64)
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    eps4, sig2, e0 = BR.atom_constants(eps, sigma, rc)
    reach = np.ceil(rc / BR.heights(cell)).astype(np.int64) + extra
    offs = np.array(list(itertools.product(*[range(-int(r), int(r) + 1) for r in reach])), dtype=np.float64)
    b = np.asarray(x, dtype=np.float64)[None, :] - static_pos
    m = np.rint(b @ np.linalg.inv(cell))[:, None, :] + offs[None, :, :]
    T = (m[..., 0:1] * cell[0] + m[..., 1:2] * cell[1]) + m[..., 2:3] * cell[2]
    d = b[:, None, :] - T
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    atom, which = np.nonzero(dd <= np.float64(rc) * np.float64(rc))
    mm = m[atom, which].astype(np.int64)
    order = np.lexsort((mm[:, 2], mm[:, 1], mm[:, 0], atom))
    atom, mm, dd = atom[order], mm[order], dd[atom, which][order]
    return BR.phi(dd, sig2[atom], eps4[atom], e0[atom]), dd, atom, mm


def flat_sum(values):
    e = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        for p in values:
            e = e + p
    return e


def energy(cell, static_pos, eps, sigma, rc, x):
    """(E(x), number of counted terms)."""
    p = voxel_terms(cell, static_pos, eps, sigma, rc, x)[0]
    return flat_sum(p), len(p)


def energies(cell, static_pos, eps, sigma, rc, grid, voxels=None):
    """``E`` at the flat voxel indices ``voxels`` (every voxel without them), float64 ``[len(voxels)]``."""
    grid = tuple(int(v) for v in grid)
    if voxels is None:
        voxels = np.arange(grid[0] * grid[1] * grid[2])
    return np.array([energy(cell, static_pos, eps, sigma, rc, center(cell, grid, unflatten(grid, int(v))))[0] for v in voxels], dtype=np.float64)


def n_tiles(grid):
    return tuple(-(-int(grid[a]) // TILE[a]) for a in range(3))


def tile_voxels(grid, t):
    """The flat voxel indices of tile ``t`` (flat over ``n_tiles``) and whether the tile is partial."""
    nt = n_tiles(grid)
    at = unflatten(nt, t)
    ranges = [range(at[a] * TILE[a], min((at[a] + 1) * TILE[a], int(grid[a]))) for a in range(3)]
    vox = [(i0 * grid[1] + i1) * grid[2] + i2 for i0 in ranges[0] for i1 in ranges[1] for i2 in ranges[2]]
    return np.array(vox, dtype=np.int64), any(len(r) < TILE[a] for a, r in enumerate(ranges))


def plan(cell, rc, grid, form=0):
    """What ``sit_landscape_plan`` answers, or ``None`` where it refuses."""
    grid = [int(v) for v in grid]
    if any(v < 1 or v > MAX_GRID for v in grid) or grid[0] * grid[1] * grid[2] > MAX_VOXELS or form not in (0, 1, 2):
        return None
    cell = np.asarray(cell, dtype=np.float64)
    if not rc > 0 or not np.isfinite(rc) or abs(np.linalg.det(cell)) == 0.0:
        return None
    q = rc / BR.heights(cell)
    if np.any(q >= 255.0):
        return None
    half = [0.5 * (min(grid[a], TILE[a]) - 1) / grid[a] for a in range(3)]
    nt = n_tiles(grid)
    out = {"tile": TILE, "threads": THREADS, "list_capacity": CHUNK, "tiles": nt[0] * nt[1] * nt[2],
           "translations": tuple(int(np.floor(v)) + 1 for v in q), "list_translations": tuple(int(np.floor(q[a] + half[a])) + 1 for a in range(3)),
           "voxels": grid[0] * grid[1] * grid[2]}
    out["form"] = form or (2 if np.all(q < 1.0) else 1)         # 0: tiled where rc is shorter than every height of the cell
    return out


# ---- the designed host: a simple tetragonal lattice, one atom per cell of edges (a, a, c), c < a, as a 2 x 2 x 2 supercell -------

TET_A, TET_C = 4.0, 2.0                # the edges of the supercell are powers of two: every centre is exact
TET_CELL = np.diag([2 * TET_A, 2 * TET_A, 2 * TET_C])
TET_GRID = (8, 8, 8)                  # 4 voxels per edge of a primitive cell: atoms, face centres and body centres are voxel centres
TET_SIGMA, TET_EPS, TET_RC = 2.5, 1.0, 4.5


def tetragonal_host():
    """(cell, static_pos [8, 3], numbers [8], grid): the atoms on the centres of the voxels ``(4 j0, 4 j1, 4 j2)``, built with the
    voxel-centre arithmetic itself."""
    pos = [center(TET_CELL, TET_GRID, (4 * j0, 4 * j1, 4 * j2)) for j0 in range(2) for j1 in range(2) for j2 in range(2)]
    return TET_CELL, np.array(pos), np.full(8, 8, dtype=np.int64), TET_GRID


def tetragonal_voxels():
    """Flat indices: (body centres [8], centres of the a x a faces [8], centres of the a x c faces [16])."""
    def flat(i):
        return (i[0] * TET_GRID[1] + i[1]) * TET_GRID[2] + i[2]
    cells = list(itertools.product(range(2), repeat=3))
    body = sorted(flat((4 * j[0] + 2, 4 * j[1] + 2, 4 * j[2] + 2)) for j in cells)
    wide = sorted(flat((4 * j[0] + 2, 4 * j[1] + 2, 4 * j[2])) for j in cells)
    narrow = sorted([flat((4 * j[0] + 2, 4 * j[1], 4 * j[2] + 2)) for j in cells] + [flat((4 * j[0], 4 * j[1] + 2, 4 * j[2] + 2)) for j in cells])
    return np.array(body), np.array(wide), np.array(narrow)
