"""A plain numpy statement of what the landmark pruning tables must contain, written from the comment at the head of
sitator_amd/csrc/candidates.hip and sharing no code with it (or with candidates_plan.h): no ctypes, no probe.

A landmark component k is non-zero only if every vertex h of k is within rz * vcd[k, h] of the ion in a metric that is
at least the periodic distance d_P, and every accepted static atom is within `displacement` of its reference position
in such a metric.  For an ion anywhere in a bin with centre c_b and covering radius rb:

    component k non-zero  =>  for all real h:  d_P(c_b, ref[v_kh]) <= rz * vcd[k, h] + displacement + rb

The MARGIN of a pair is  m(b, k) = min_h [ rz * vcd[k, h] + displacement + rb_true - d_P(c_b, ref[v_kh]) ]  and a table
is right when it lists every pair with m >= 0 (complete) and nothing with m below minus the pads the code adds.

d_P is an exhaustive minimum over the images [-N, N]^3 of the round-reduced fractional difference, with
N = ceil(T_max / h_min) + 1 taken from the case: an image further out along axis i is at least (N + 1 - 0.5) h_i > T_max
away.  Everything is float64; the pads below say what that costs."""
import numpy as np

MAX_GRID = 192
MAX_BINS = 1500000
PAD_ABS = 1e-6 + 1e-9            # `rb += 1e-6` and the `+ 1e-9` of bound_of
PAD_REL = 1e-9                   # the two (1 + 1e-9) factors of bound_of
REF_EPS = 1e-9                   # the reference's own rounding (positions of ~1e2 A in float64: ~1e-13; generous)


def heights(cell):
    """Perpendicular heights: h_i = distance between the lattice planes of axis i = 1 / |b_i|, b_i the columns of the
    inverse cell (rows of the cell are the lattice vectors)."""
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(cell, dtype=np.float64)), axis=0)


def grid_of(cell, bin_target):
    """round(len / bin_target) per axis (halves away from zero), clamped to [1, 192], the largest axis thinned by 3/4
    while there are more than 1 500 000 bins."""
    length = np.linalg.norm(np.asarray(cell, dtype=np.float64), axis=1)
    G = [int(min(max(np.floor(x / bin_target + 0.5), 1), MAX_GRID)) for x in length]
    while G[0] * G[1] * G[2] > MAX_BINS:
        m = 0 if (G[0] >= G[1] and G[0] >= G[2]) else (1 if G[1] >= G[2] else 2)
        G[m] = G[m] * 3 // 4
    return G


def covering_radius(cell, G):
    """Half the longest of the four body diagonals of one bin (edges cell[i] / G[i])."""
    e = np.asarray(cell, dtype=np.float64) / np.asarray(G, dtype=np.float64)[:, None]
    return 0.5 * max(np.linalg.norm(e[0] + sa * e[1] + sb * e[2]) for sa in (-1, 1) for sb in (-1, 1))


def bin_centres(cell, G):
    """[nb, 3]; bin (x, y, z) is row (x * G[1] + y) * G[2] + z, its centre ((i + 0.5) / G) @ cell."""
    ix, iy, iz = np.meshgrid(np.arange(G[0]), np.arange(G[1]), np.arange(G[2]), indexing="ij")
    frac = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) + 0.5) / np.asarray(G, dtype=np.float64)
    return frac @ np.asarray(cell, dtype=np.float64)


def periodic_distance(cell, a, b, T_max, exact_below=None):
    """d_P between the points a [n, 3] and ONE point b: reduce the fractional difference by round, then the minimum norm
    over all images in [-N, N]^3, N = ceil(T_max / h_min) + 1.

    exact_below (large grids only; "auto" in Reference = T_max + 1): pairs for which max_i |f_i| h_i - a lower bound of d_P, because no image has a
    smaller |f_i| than the reduced one and a vector with fractional coordinate g is at least |g| h_i long - exceeds it
    are not searched; that lower bound is returned for them (their margin comes out too HIGH, never too low)."""
    cell = np.asarray(cell, dtype=np.float64)
    h = heights(cell)
    N = int(np.ceil(T_max / h.min())) + 1
    f = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) @ np.linalg.inv(cell)
    f -= np.round(f)
    lower = np.max(np.abs(f) * h, axis=1)
    out = lower.copy()
    sel = np.arange(len(f)) if exact_below is None else np.nonzero(lower <= exact_below)[0]
    if len(sel) == 0:
        return out
    fs = f[sel]
    best = np.full(len(sel), np.inf)
    rng = np.arange(-N, N + 1)
    for i in rng:
        for j in rng:
            g = fs[:, None, :] + np.stack([np.full(len(rng), i), np.full(len(rng), j), rng], axis=1)[None, :, :]
            r = g @ cell
            best = np.minimum(best, np.sqrt(np.einsum("nik,nik->ni", r, r)).min(axis=1))
    out[sel] = best
    return out


class Reference(object):
    """Margins of every (bin, landmark) pair of a case for a table with the given grid and displacement."""

    def __init__(self, cell, ref_static, verts, vcd, rz, displacement, G, exact_below=None):
        self.cell = np.asarray(cell, dtype=np.float64)
        self.verts = np.asarray(verts, dtype=np.int64)
        self.real = self.verts >= 0
        self.nv = self.real.sum(axis=1)
        assert np.array_equal(self.real, np.arange(self.verts.shape[1])[None, :] < self.nv[:, None]), "-1 only as padding"
        self.reach = np.where(self.real, rz * np.where(self.real, vcd, 0.0), -np.inf)      # rz * vcd[k, h]
        self.G = [int(g) for g in G]
        self.nb = self.G[0] * self.G[1] * self.G[2]
        self.D = len(self.verts)
        self.displacement = float(displacement)
        self.rb_true = covering_radius(self.cell, self.G)
        self.T_max = float(self.reach.max() + self.displacement + self.rb_true)
        if isinstance(exact_below, str):                     # "auto": a pair that far out has a margin below -1
            exact_below = self.T_max + 1.0
        self.centres = bin_centres(self.cell, self.G)
        used = np.unique(self.verts[self.real])
        # d[b, s]: the periodic distance between every bin centre and every static atom that is a vertex
        self.dist = np.full((self.nb, len(ref_static)), np.nan)
        for s in used:
            self.dist[:, s] = periodic_distance(self.cell, self.centres, ref_static[s], self.T_max, exact_below)
        d = self.dist[:, np.where(self.real, self.verts, used[0])]                          # [nb, D, V]
        self.vertex_distance = np.where(self.real[None], d, -np.inf)
        room = np.where(self.real[None], self.reach[None] + self.displacement + self.rb_true - d, np.inf)
        self.margin = room.min(axis=2)                                                      # [nb, D]
        self.pad = PAD_ABS + PAD_REL * (np.where(self.nv > 0, self.reach.max(axis=1), 0.0) + self.displacement)     # [D]

    def images_per_axis(self):
        """floor(T / h + 0.5) for the largest bound of the case: what the code's image search needs per axis."""
        return np.floor(self.T_max / heights(self.cell) + 0.5).astype(int)


def check_table(ref, table, W=None, mean=None, label=""):
    """`table`: dict with grid, displacement, rb, total, off, list, crit.  Asserts completeness, no padding beyond the
    code's pads, structure and the critical vertices; returns (listed, undecided, share of undecided pairs)."""
    off = np.asarray(table["off"], dtype=np.int64)
    lst = np.asarray(table["list"], dtype=np.int64)
    crit = np.asarray(table["crit"], dtype=np.int64)
    total = int(table["total"])
    assert [int(g) for g in table["grid"]] == ref.G, (label, table["grid"], ref.G)
    # ---- structure
    assert len(off) == ref.nb + 1 and off[0] == 0 and off[-1] == total == len(lst) == len(crit), label
    length = np.diff(off)
    assert (length >= 0).all(), label
    bins = np.repeat(np.arange(ref.nb), length)
    assert ((lst >= 0) & (lst < ref.D)).all(), label
    inner = np.ones(total, dtype=bool)
    inner[off[:-1][length > 0]] = False                               # not the first entry of its bin
    assert (np.diff(lst)[inner[1:]] > 0).all(), "%s: a bin's list is not strictly ascending" % label
    assert (crit < np.maximum(ref.nv[lst], 1)).all(), "%s: a critical vertex beyond the landmark's vertices" % label
    if W is not None:
        assert int(W) == (int(length.max()) if total else 1), (label, W, length.max())
    if mean is not None:
        assert mean == total / ref.nb, (label, mean, total / ref.nb)
    # ---- the bound
    listed = np.zeros((ref.nb, ref.D), dtype=bool)
    listed[bins, lst] = True
    missing = np.argwhere((ref.margin >= 0) & ~listed)
    assert len(missing) == 0, "%s: INCOMPLETE - %d pairs with margin >= 0 are not listed; first (bin %d, landmark %d) margin %.3e" % (
        label, len(missing), missing[0][0], missing[0][1], ref.margin[missing[0][0], missing[0][1]])
    floor_ = -ref.pad[None, :] - REF_EPS
    padded = np.argwhere(listed & (ref.margin < floor_))
    assert len(padded) == 0, "%s: %d listed pairs lie beyond the code's pads; first (bin %d, landmark %d) margin %.3e" % (
        label, len(padded), padded[0][0] if len(padded) else -1, padded[0][1] if len(padded) else -1,
        ref.margin[padded[0][0], padded[0][1]] if len(padded) else 0)
    undecided = int(((ref.margin < 0) & (ref.margin >= floor_)).sum())
    share = undecided / max(total, 1)
    assert share < 1e-3, "%s: %d of %d pairs inside the pads - move an atom off the band" % (label, undecided, total)
    # ---- critical vertex: its room is the smallest of the pair (to 1e-9; which index is free)
    if total:
        bound = ref.reach[lst] * (1.0 + 1e-9) + table["displacement"] * (1.0 + 1e-9) + table["rb"] + 1e-9      # [total, V]
        real = ref.real[lst]
        room = np.where(real, np.where(real, bound, 0.0) - np.where(real, ref.vertex_distance[bins, lst], 0.0), np.inf)
        chosen = room[np.arange(total), crit]
        assert (chosen <= room.min(axis=1) + 1e-9).all(), "%s: a critical vertex is not the one with the least room" % label
    return total, undecided, share
