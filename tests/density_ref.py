"""The numpy restatement of sitator_amd/csrc/density_plan.h and of what density.hip counts, smooths and picks (DESIGN.md section
23): the same float64 operations in the same order - every ``*``, ``+`` and ``-`` below is one rounded operation, as under
-ffp-contract=off - and integer counts, so that the device's arrays are compared on their bytes."""
import itertools

import numpy as np

THREADS = 256
MAX_GRID = 1024
MAX_CLASSES = 16
MAX_CELLS = 1 << 27
MAX_F = 1 << 29
MAX_ATOMS = 1 << 20
MAX_TAPS = 1 << 15
RUN = 64
SLOT_BITS = 12
SLOTS = 1 << SLOT_BITS
PROBE = 16
TILE = (4, 8, 8)
SMOOTH_LDS = 61440
DEFAULT_WORKSPACE = 1 << 30
U = 2.0 ** -53


def cell_inverse(cell):
    """``ci`` as a context carries it: numpy's inverse of ``cell^T``."""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(cell, dtype=np.float64).T))


def frac(ci, a, x, y, z):
    """``msd_frac``: the row of ``ci`` summed left to right."""
    return (ci[a, 0] * x + ci[a, 1] * y) + ci[a, 2] * z


def axis_index(s, n):
    """``dn_axis``: int64, -1 where ``s`` is not finite."""
    s = np.asarray(s, dtype=np.float64)
    ok = np.isfinite(s)
    safe = np.where(ok, s, 0.0)
    f = safe - np.floor(safe)
    g = f * np.float64(n)
    i = g.astype(np.int64)
    i = np.where(i >= n, n - 1, i)
    return np.where(ok, i, -1)


def voxel(points, ci, grid):
    """``dn_voxel`` of ``points [..., 3]``: int64, -1 for a point in no voxel."""
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        i = [axis_index(frac(ci, a, x, y, z), int(grid[a])) for a in range(3)]
    v = (i[0] * int(grid[1]) + i[1]) * int(grid[2]) + i[2]
    return np.where((i[0] < 0) | (i[1] < 0) | (i[2] < 0), -1, v)


def plane(labels, site_class, n_classes):
    """``dn_plane`` of labels in ``[-1, K)``."""
    labels = np.asarray(labels, dtype=np.int64)
    sc = np.asarray(site_class, dtype=np.int64)
    return np.where(labels < 0, n_classes - 1, sc[np.clip(labels, 0, len(sc) - 1)])


def counts(positions, cell, atoms, grid, frame_stride=1, labels=None, site_class=None, n_classes=1):
    """``(counts uint64 [n_classes, n0, n1, n2], frames taken, skipped)`` of ``positions [F, A, 3]``; ``labels [F, n_sel]``."""
    ci = cell_inverse(cell)
    grid = [int(v) for v in grid]
    V = grid[0] * grid[1] * grid[2]
    taken = np.arange(0, len(positions), frame_stride)
    v = voxel(np.asarray(positions)[taken][:, np.asarray(atoms, dtype=np.int64)], ci, grid)
    pl = np.zeros_like(v) if labels is None else plane(np.asarray(labels)[taken], site_class, n_classes)
    out = np.zeros(n_classes * V, dtype=np.uint64)
    ok = v >= 0
    np.add.at(out, (pl * V + v)[ok], np.uint64(1))
    return out.reshape([n_classes] + grid), len(taken), int((~ok).sum())


def smooth(cnt, taps, weights):
    """The rolled grids accumulated in tap order from +0: ``out[p][i] = sum_k w_k * float64(cnt[p][(i + d_k) mod n])``."""
    c = np.asarray(cnt).astype(np.float64)
    out = np.zeros_like(c)
    for d, w in zip(np.asarray(taps, dtype=np.int64), np.asarray(weights, dtype=np.float64)):
        out = out + np.float64(w) * np.roll(c, (-int(d[0]), -int(d[1]), -int(d[2])), axis=(-3, -2, -1))
    return out


def neighbours(v, grid):
    """The periodic neighbours ``u != v`` of voxel ``v`` (with repetitions where an axis is short)."""
    n0, n1, n2 = grid
    i0, i1, i2 = v // (n1 * n2), (v // n2) % n1, v % n2
    out = []
    for d in itertools.product((-1, 0, 1), repeat=3):
        u = (((i0 + d[0]) % n0) * n1 + (i1 + d[1]) % n1) * n2 + (i2 + d[2]) % n2
        if u != v:
            out.append(u)
    return out


def is_peak(flat, grid, v, threshold):
    c = flat[v]
    if not c >= threshold:
        return False
    return all(flat[u] < c or (flat[u] == c and u > v) for u in neighbours(v, grid))


def peaks(grid_values, threshold):
    """The peak rule by brute force: int64 voxel indices, ascending."""
    g = np.asarray(grid_values, dtype=np.float64)
    flat = g.reshape(-1)
    return np.array([v for v in range(flat.size) if is_peak(flat, g.shape, v, threshold)], dtype=np.int64)


def slot(key):
    return ((int(key) * 2654435761) & 0xFFFFFFFF) >> (32 - SLOT_BITS)


def probe(first, i):
    return (first + i) & (SLOTS - 1)


def halo(taps, grid):
    """``dn_halo``: the largest ``|d_a|``, or ``None`` for a tap beyond ``(n_a - 1) // 2``."""
    t = np.asarray(taps, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return [0, 0, 0]
    h = np.abs(t).max(axis=0)
    if any(int(h[a]) > (int(grid[a]) - 1) // 2 for a in range(3)):
        return None
    return [int(v) for v in h]


def gaussian_stencil(cell, grid, sigma, cutoff=4.0):
    """Brute force: every offset of a generous box, kept where its Cartesian length is at most ``cutoff * sigma``."""
    cell = np.asarray(cell, dtype=np.float64)
    steps = cell / np.asarray(grid, dtype=np.float64)[:, None]
    r_max = cutoff * sigma
    # a box sized without the operator's bound: |d . steps| >= |d| sigma_min(steps), so no offset beyond r_max / sigma_min counts
    most = int(np.ceil(r_max / np.linalg.svd(steps, compute_uv=False).min())) + 2
    reach = [most, most, most]
    taps, r2 = [], []
    for d in itertools.product(*(range(-m, m + 1) for m in reach)):
        vec = d[0] * steps[0] + d[1] * steps[1] + d[2] * steps[2]
        if np.sqrt(vec @ vec) <= r_max:
            taps.append(d)
            r2.append(vec @ vec)
    taps = np.array(taps, dtype=np.int64).reshape(-1, 3)
    if np.any(np.abs(taps).max(axis=0) > (np.asarray(grid) - 1) // 2) or len(taps) > MAX_TAPS:
        raise ValueError("the stencil does not fit the grid")
    w = np.exp(-np.array(r2) / (2.0 * sigma * sigma))
    return taps, w / w.sum()


def round_up(v, m):
    return (v + m - 1) // m * m


def plan(F, A, n_sel, grid, stride=1, K=0, n_classes=1, n_taps=0, halo3=(0, 0, 0), form=0, host=True, cap=0):
    """``dn_plan``: a dict, or ``None`` where it refuses."""
    n = [int(v) for v in grid]
    if any(v < 1 or v > MAX_GRID for v in n) or not (1 <= n_classes <= MAX_CLASSES) or K < 0 or (K > 0 and n_classes < 2):
        return None
    V = n[0] * n[1] * n[2]
    cells = n_classes * V
    if cells > MAX_CELLS or not (1 <= F <= MAX_F) or stride < 1 or not (1 <= n_sel <= MAX_ATOMS) or A < 1 or not (0 <= n_taps <= MAX_TAPS):
        return None
    if any(halo3[a] < 0 or halo3[a] > (n[a] - 1) // 2 for a in range(3)) or form not in (0, 1, 2) or cap < 0:
        return None
    taken = (F - 1) // stride + 1
    p = dict(V=V, cells=cells, taken=taken, runs=-(-taken // RUN), lds_bytes=SLOTS * 8 + 24)
    p["form"] = form or (2 if cells <= SLOTS else 1)               # every key has a slot of its own: the table; else direct
    if host:
        cap = (cap if cap > 0 else DEFAULT_WORKSPACE) & ~255
        most = cap // (A * 24)
        first = min(taken, RUN)
        if most < (first - 1) * stride + 1:
            return None
        w = (most - 1) // stride + 1
        p["window"] = taken if w >= taken else w // RUN * RUN
    else:
        p["window"] = taken
    p["n_windows"] = -(-taken // p["window"])
    p["window_frames"] = (p["window"] - 1) * stride + 1
    p["ext"] = [TILE[a] + 2 * int(halo3[a]) for a in range(3)]
    ext_bytes = p["ext"][0] * p["ext"][1] * p["ext"][2] * 8
    p["smooth_lds"] = ext_bytes if n_taps > 0 and ext_bytes <= SMOOTH_LDS else 0
    p["workspace"] = round_up(round_up(p["window_frames"] * A * 24, 16), 256) if host else 0
    return p
