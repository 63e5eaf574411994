"""``DensityPercolation``: at which iso-level does the density of the mobile ions first connect across the periodic cell, and in how
many dimensions (no counterpart in the reference; ``DESIGN.md`` section 24).  ``-kT ln(t_d / rho_max)`` at that level is the density
estimate of the migration barrier; the rank tells whether conduction is 1-D, 2-D or 3-D.  It is the density's version of what
``DiffusionPathwayAnalysis`` answers on the site graph, and needs no fitted sites.

The connected components of a superlevel set ``{g >= level}`` are labelled by HIP kernels (``sit_percolation_components``, bound in
``_lib_percolation.py``); every component comes with the rank and the Hermite normal form of its loop lattice - the integer
combinations of cell vectors it is unbounded along.  ``sit_percolation_levels`` bisects for the three levels on the device-resident
grid."""
import numpy as np

from . import _lib


def _with_ctx(cell, ctx, call):
    if ctx is not None:
        return call(ctx)
    with _lib.HipContext(np.asarray(cell, dtype=np.float64)) as own:
        return call(own)


class ComponentsResult(object):
    """The components of ``{grid >= level}``.  ``labels`` int32 of the grid's shape: the lowest flat index of the voxel's component,
    -1 outside the set; ``roots`` int32 ``[n]`` ascending, ``sizes`` int64 ``[n]`` voxels; ``rank`` int32 ``[n]`` and ``basis`` int32
    ``[n, 3, 3]``: the rank and the row Hermite normal form of the lattice of cell translations the component runs into itself by;
    ``rounds``, ``seam_records``: what the labelling took."""

    def __init__(self, grid, cell, level, connectivity, labels, records, info):
        self.grid_values = grid
        self.cell = np.asarray(cell, dtype=np.float64)
        self.level, self.connectivity = float(level), int(connectivity)
        self.labels = labels
        self.roots = np.ascontiguousarray(records[:, 0], dtype=np.int32)
        self.sizes = np.ascontiguousarray(records[:, 1])
        self.rank = np.ascontiguousarray(records[:, 2], dtype=np.int32)
        self.basis = np.ascontiguousarray(records[:, 3:12], dtype=np.int32).reshape(-1, 3, 3)
        self.rounds, self.seam_records, self.form = info[0], info[1], info[2]

    @property
    def grid(self):
        return tuple(int(v) for v in self.labels.shape)

    @property
    def directions(self):
        """``[n, 3, 3]``: ``basis @ cell``, the Cartesian translations of every component (zero rows beyond its rank)."""
        return self.basis.astype(np.float64) @ self.cell

    @property
    def mass(self):
        """``[n]``: the sum of the grid over every component's voxels (on the host)."""
        flat, values = self.labels.reshape(-1), self.grid_values.reshape(-1)
        inside = flat >= 0
        total = np.bincount(flat[inside], weights=values[inside], minlength=flat.size)
        return total[self.roots]

    def _rank_of_label(self):
        table = np.zeros(self.labels.size + 1, dtype=np.int32)      # slot -1: outside the set
        table[self.roots] = self.rank
        return table

    def percolating(self, d=1):
        """A boolean mask of the grid's shape: the voxels of the components of rank >= ``d``."""
        return self._rank_of_label()[self.labels] >= int(d)

    def sites(self, sn, d=1):
        """``(labels int32 [n_sites], on_pathway bool [n_sites])``: the label of the voxel every site centre of ``sn`` lies in
        (the voxel rule of ``DensityResult.voxel_of``; -1 outside the set) and whether that component has rank >= ``d`` - the
        counterpart of the pathway sites of ``DiffusionPathwayAnalysis``."""
        from .density import voxel_of
        lab = self.labels.reshape(-1)[voxel_of(self.cell, self.grid, np.asarray(sn.centers, dtype=np.float64))]
        return lab, self._rank_of_label()[lab] >= int(d)


class PercolationResult(object):
    """``levels`` float64 ``[3]``: ``t_1 >= t_2 >= t_3``, the largest positive grid value at which the superlevel set has a component
    of rank >= 1, 2, 3 (0.0: not even ``{g > 0}`` has one); ``ranks`` int32 ``[3]``: the largest rank present at that level;
    ``passes``: labelling passes of the search; ``top``: the largest grid value."""

    def __init__(self, levels, ranks, info, top):
        self.levels, self.ranks = levels, ranks
        self.passes, self.rounds, self.seam_records, self.form = info
        self.top = float(top)

    @property
    def dimensionality(self):
        """The largest ``d`` with ``t_d > 0``; 0 where the density percolates nowhere."""
        return int((self.levels > 0.0).sum())

    def barriers(self, kT):
        """``-kT ln(t_d / max g)`` for ``d`` = 1, 2, 3; ``inf`` where ``t_d == 0``."""
        out = np.full(3, np.inf)
        ok = self.levels > 0.0
        out[ok] = -float(kT) * np.log(self.levels[ok] / self.top)
        return out


def density_components(grid, cell, level, connectivity=26, ctx=None, form=0):
    """The components of ``{grid >= level}`` of a 3-D float64 array over the periodic ``cell`` (rows are the cell vectors), as a
    ``ComponentsResult``.  ``ctx``: a ``HipContext`` to run on (any: the labelling does not look at its cell); without it one is made
    for the call."""
    from . import _lib_percolation
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    labels, records, info = _with_ctx(cell, ctx, lambda c: _lib_percolation.percolation_components(c, grid, level, connectivity, form))
    return ComponentsResult(grid, cell, level, connectivity, labels, records, info)


def density_percolation(grid, cell, connectivity=26, ctx=None, form=0):
    """The percolation levels of a 3-D float64 array over the periodic ``cell``, as a ``PercolationResult``."""
    from . import _lib_percolation
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    levels, ranks, info = _with_ctx(cell, ctx, lambda c: _lib_percolation.percolation_levels(c, grid, connectivity, form))
    positive = grid[grid > 0.0]
    return PercolationResult(levels, ranks, info, positive.max() if positive.size else 0.0)
