"""A restatement of DensityPercolation that shares no code with sitator_amd/csrc/percolation_plan.h: a
breadth-first walk per component that gives every voxel an integer image potential, a loop vector wherever a visited voxel is met
at a different potential, rank and Hermite normal form by exact (Python) integer arithmetic, and the levels by evaluating the
predicate at the sorted distinct positive values.  tests/test_percolation_ref.py holds it to designed answers."""
import functools
import itertools
from collections import deque

import numpy as np

THREADS = 256
TILE = (8, 8, 16)
MAX_GRID = 1024
MAX_VOXELS = 1 << 27


def offsets(connectivity):
    """The offsets of a connectivity, in lexicographic order."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(x != 0 for x in d) <= most]


def neighbour(i, d, n):
    """``(j, s)``: the neighbour ``(i + d) mod n`` and the shift ``floor((i + d) / n)``, per axis."""
    return tuple((i[a] + d[a]) % n[a] for a in range(3)), tuple((i[a] + d[a]) // n[a] for a in range(3))


def hnf(vectors):
    """The row Hermite normal form of the lattice the integer 3-vectors generate, as a 3 x 3 list of Python ints (zero rows last),
    and its rank."""
    rows = [[int(x) for x in v] for v in vectors if any(int(x) != 0 for x in v)]
    basis = []
    for c in range(3):
        while True:                                                  # Euclid among the rows that are non-zero in column c
            live = [r for r in rows if r[c] != 0]
            if len(live) <= 1:
                break
            live.sort(key=lambda r: abs(r[c]))
            small = live[0]
            for r in live[1:]:
                q = r[c] // small[c]
                for k in range(3):
                    r[k] -= q * small[k]
        live = [r for r in rows if r[c] != 0]
        if live:
            p = live[0]
            rows = [r for r in rows if r is not p]
            if p[c] < 0:
                p = [-x for x in p]
            basis.append((c, p))
        rows = [r for r in rows if any(r)]
    for a in range(len(basis)):                                      # entries above a pivot into [0, pivot)
        for b in range(a + 1, len(basis)):
            c, p = basis[b]
            q = basis[a][1][c] // p[c]
            basis[a] = (basis[a][0], [x - q * y for x, y in zip(basis[a][1], p)])
    out = [p for _, p in basis]
    rank = len(out)
    return out + [[0, 0, 0]] * (3 - rank), rank


@functools.lru_cache(maxsize=8)
def _tables(n, connectivity):
    """Per offset: the neighbour's flat index and the three shifts of every voxel, as lists."""
    idx = np.indices(n).reshape(3, -1)
    out = []
    for d in offsets(connectivity):
        j = [(idx[a] + d[a]) % n[a] for a in range(3)]
        s = [((idx[a] + d[a]) // n[a]).tolist() for a in range(3)]
        out.append((np.ravel_multi_index(j, n).tolist(), s[0], s[1], s[2]))
    return out


def components(grid, level, connectivity=26):
    """``(labels int32 of the grid's shape, roots, sizes, rank, basis [n, 3, 3])`` of ``{grid >= level}``."""
    grid = np.asarray(grid, dtype=np.float64)
    n = tuple(int(v) for v in grid.shape)
    with np.errstate(invalid="ignore"):
        inside = (grid >= level).reshape(-1)
    tables = _tables(n, connectivity)
    ins = inside.tolist()
    V = len(ins)
    label = [-1] * V
    p0, p1, p2 = [0] * V, [0] * V, [0] * V
    roots, sizes, ranks, bases = [], [], [], []
    for root in np.flatnonzero(inside).tolist():                     # ascending flat index: the first voxel met is the lowest
        if label[root] >= 0:
            continue
        label[root] = root
        queue, size, loops = deque([root]), 0, set()
        while queue:
            i = queue.popleft()
            size += 1
            for nbr, s0, s1, s2 in tables:
                j = nbr[i]
                if not ins[j]:
                    continue
                q0, q1, q2 = p0[i] + s0[i], p1[i] + s1[i], p2[i] + s2[i]
                if label[j] < 0:
                    label[j] = root
                    p0[j], p1[j], p2[j] = q0, q1, q2
                    queue.append(j)
                elif (p0[j], p1[j], p2[j]) != (q0, q1, q2):
                    loops.add((q0 - p0[j], q1 - p1[j], q2 - p2[j]))
        basis, rank = hnf(sorted(loops))
        roots.append(root), sizes.append(size), ranks.append(rank), bases.append(basis)
    return (np.array(label, dtype=np.int32).reshape(n), np.array(roots, dtype=np.int32), np.array(sizes, dtype=np.int64),
            np.array(ranks, dtype=np.int32), np.array(bases, dtype=np.int32).reshape(-1, 3, 3))


def max_rank(grid, level, connectivity=26):
    r = components(grid, level, connectivity)[3]
    return int(r.max()) if len(r) else 0


def levels(grid, connectivity=26):
    """``(levels float64 [3], ranks int32 [3])``: the predicate at every distinct positive value, from the largest down."""
    grid = np.asarray(grid, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        values = np.unique(grid[grid > 0.0])[::-1]
    t, r = np.zeros(3), np.zeros(3, dtype=np.int32)
    found = 0
    for v in values:
        rank = max_rank(grid, v, connectivity)
        while found < rank:
            t[found], r[found] = v, rank
            found += 1
        if found == 3:
            break
    return t, r


def snap(grid, lo):
    """``min{g : g > 0 and g >= lo}``, or ``None``."""
    grid = np.asarray(grid, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = grid[(grid > 0.0) & (grid >= lo)]
    return float(c.min()) if c.size else None


def seam_max(n, connectivity):
    """Seam edges of the full grid, every undirected one once: from the end that sees the lexicographically positive shift."""
    total = 0
    for d in offsets(connectivity):
        per_axis = []
        for a in range(3):
            shifts = [(i + d[a]) // n[a] for i in range(n[a])]
            per_axis.append({s: shifts.count(s) for s in (-1, 0, 1)})
        for s in itertools.product((-1, 0, 1), repeat=3):
            if s > (0, 0, 0):
                total += per_axis[0][s[0]] * per_axis[1][s[1]] * per_axis[2][s[2]]
    return total


def align(x, a=256):
    return -(-x // a) * a


def piece(count, size):
    return -(-(max(count, 0) * size) // 16) * 16


def plan(n, connectivity=26, form=0):
    """What ``pc_plan`` gives, or ``None`` where it refuses."""
    if any(v < 1 or v > MAX_GRID for v in n):
        return None
    V = n[0] * n[1] * n[2]
    if V > MAX_VOXELS or connectivity not in (6, 18, 26) or form not in (0, 1, 2):
        return None
    tiles = [-(-n[a] // TILE[a]) for a in range(3)]
    seam = seam_max(n, connectivity)
    used = 0
    for count, size in ((V, 8), (V, 4), (16, 8), (3 * seam, 4)):
        used = align(used) + piece(count, size)
    return dict(V=V, n_tiles=tiles[0] * tiles[1] * tiles[2], lds_bytes=4 * TILE[0] * TILE[1] * TILE[2], seam_max=seam,
                form=form or 2, blocks=-(-V // THREADS), workspace=align(used))


# ---- designed grids: what the set is, and what must come out ---------------------------------------------------------------------

E = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
STRAND_A = [(1, 1), (1, 1), (1, 1), (1, 1), (1, 2), (1, 3), (2, 3), (3, 3)]      # the transverse place of the first lap at i0 = 0 .. 7
STRAND_B = [(3, 3), (3, 3), (3, 3), (3, 3), (3, 2), (3, 1), (2, 1), (1, 1)]      # ... of the second: the two change places without touching


def _basis(*rows):
    rows = [list(r) for r in rows]
    return rows + [[0, 0, 0]] * (3 - len(rows))


def designed():
    """``[(name, grid, level, connectivity, [(size, rank, basis)] by ascending root)]``: sets whose components can be read off."""
    out = []

    def add(name, shape, voxels, connectivity, expected, level=1.0):
        g = np.zeros(shape)
        for v in voxels:
            g[v] = 1.0
        out.append((name, g, level, connectivity, expected))

    n = (5, 6, 7)
    for a in range(3):
        line = [tuple(k if b == a else (2, 3, 4)[b] for b in range(3)) for k in range(n[a])]
        add("channel_along_%d" % a, n, line, 6, [(n[a], 1, _basis(E[a]))])
    diag = [(i, i, 1) for i in range(6)]
    add("diagonal_1_1_0", (6, 6, 4), diag, 18, [(6, 1, _basis([1, 1, 0]))])
    add("diagonal_1_1_0_by_faces", (6, 6, 4), diag, 6, [(1, 0, _basis())] * 6)
    add("winding_1_2_0", (6, 3, 4), [(i, i % 3, 1) for i in range(6)], 26, [(6, 1, _basis([1, 2, 0]))])
    helix = [(i, ) + STRAND_A[i] for i in range(8)] + [(i, ) + STRAND_B[i] for i in range(8)]
    add("double_loop_2_0_0", (8, 5, 5), helix, 26, [(16, 1, _basis([2, 0, 0]))])
    add("plane", n, [(2, j, k) for j in range(6) for k in range(7)], 6, [(42, 2, _basis(E[1], E[2]))])
    add("full", n, [(i, j, k) for i in range(5) for j in range(6) for k in range(7)], 6, [(210, 3, _basis(*E))])
    add("two_channels", n, [(i, 1, 1) for i in range(5)] + [(3, j, 4) for j in range(6)], 26,
        [(5, 1, _basis(E[0])), (6, 1, _basis(E[1]))])
    add("corner_channel_26", (4, 4, 4), [(i, i, i) for i in range(4)], 26, [(4, 1, _basis([1, 1, 1]))])
    add("corner_channel_18", (4, 4, 4), [(i, i, i) for i in range(4)], 18, [(1, 0, _basis())] * 4)
    add("corner_channel_6", (4, 4, 4), [(i, i, i) for i in range(4)], 6, [(1, 0, _basis())] * 4)
    add("one_voxel_grid", (1, 1, 1), [(0, 0, 0)], 6, [(1, 3, _basis(*E))])
    add("axis_of_one", (1, 4, 4), [(0, 1, 2)], 26, [(1, 1, _basis(E[0]))])
    add("axis_of_two_one_voxel", (2, 4, 4), [(1, 1, 2)], 26, [(1, 0, _basis())])
    add("axis_of_two_both", (2, 4, 4), [(0, 1, 2), (1, 1, 2)], 6, [(2, 1, _basis(E[0]))])
    add("two_three_five_full", (2, 3, 5), [(i, j, k) for i in range(2) for j in range(3) for k in range(5)], 18, [(30, 3, _basis(*E))])
    return out
