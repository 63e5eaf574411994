"""``EnergyLandscape``: the energy of one probe ion at the centre of every voxel of a grid over the periodic cell, in the frozen
lattice of the static atoms (no counterpart in the reference; ``DESIGN.md`` section 25) - the static answer to what ``IonicDensity``
and ``DensityResult.percolation`` answer from a trajectory: where can a mobile ion sit, and what does it cost it to get across the
cell.  It needs no MD run, and it sees the saddles a short or cold run never sampled.

The energies come from HIP kernels (``sit_landscape_energies``, bound in ``_lib_landscape.py``) under the truncated and shifted 12-6
potential a ``sitator_amd.calculators.LennardJones`` describes, as ``MergeSitesByBarrier`` uses it.  The minima are the peaks
(``sit_density_peaks``) and the static barriers the percolation levels (``sit_percolation_levels``) of the energies turned over,
``g = e_cap - E``: a monotone map onto the positive values those calls work on."""
import numpy as np

from . import _lib
from .calculators import LennardJones
from .density import BOHR, MAX_GRID, _voxel_vectors, voxel_of
from .pbc import PBCCalculator
from .percolation import PercolationResult, _with_ctx, density_components, density_percolation


class LandscapeResult(object):
    """What ``EnergyLandscape`` returns.  ``energies`` float64 ``[n0, n1, n2]``: the energy at every voxel centre in the units of
    ``epsilon``, ``+inf`` on an atom; ``cell``, ``grid``; ``e_min``, the lowest energy; ``form``, ``tiles``, ``list_chunks``,
    ``candidate_terms``: what the evaluation took."""

    def __init__(self, energies, cell, info=(0, 0, 0, 0)):
        self.energies = energies
        self.cell = np.asarray(cell, dtype=np.float64)
        self.grid = tuple(int(v) for v in energies.shape)
        self.e_min = float(energies.min())
        self.form, self.tiles, self.list_chunks, self.candidate_terms = (int(v) for v in info)

    def fractional_centers(self):
        """``[n0, n1, n2, 3]``: ``f_a = (i_a + 0.5) / n_a``, the fractional coordinates of the voxel centres."""
        axes = [(np.arange(n).astype(np.float64) + 0.5) / float(n) for n in self.grid]
        return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)

    def cartesian_centers(self):
        """``[n0, n1, n2, 3]``: ``x_k = (f0 cell[0][k] + f1 cell[1][k]) + f2 cell[2][k]``, the rule of the kernels and in their
        order - not a matrix product."""
        f, c = self.fractional_centers(), self.cell
        return (f[..., 0:1] * c[0] + f[..., 1:2] * c[1]) + f[..., 2:3] * c[2]

    def _cap(self, e_cap):
        if e_cap is not None:
            return float(e_cap)
        finite = self.energies[np.isfinite(self.energies)]
        return float(finite.max()) if finite.size else 0.0

    def capped(self, e_cap=None):
        """``g = e_cap - E`` where ``E < e_cap``, else 0.0: positive exactly below the cap and non-increasing in ``E``.  ``e_cap``
        defaults to the largest finite energy."""
        cap = self._cap(e_cap)
        g = np.zeros(self.energies.shape)
        below = self.energies < cap
        g[below] = cap - self.energies[below]
        return g

    def minima(self, window=None, ctx=None):
        """``(voxels int64 [n], fractional [n, 3], cartesian [n, 3], energies [n])``: the voxels whose energy lies below that of
        their 26 periodic neighbours (equal energies: the lowest index wins) and below ``e_min + window`` (``None``: below the
        largest finite energy), found on the device, sorted by energy ascending with ties by index."""
        from . import _lib_density
        g = self.capped(None if window is None else self.e_min + float(window))
        tiny = np.nextafter(0.0, 1.0)                              # every positive value passes
        v = _with_ctx(self.cell, ctx, lambda c: _lib_density.density_peaks(c, g, tiny))
        e = self.energies.reshape(-1)[v]
        order = np.lexsort((v, e))
        v, e = v[order], e[order]
        return v, self.fractional_centers().reshape(-1, 3)[v], self.cartesian_centers().reshape(-1, 3)[v], e

    def components(self, energy, connectivity=26, e_cap=None, ctx=None):
        """The connected components of ``{E <= energy}`` (below the cap), with the rank and the basis of every component's loop
        lattice: a ``ComponentsResult`` on the capped grid at the level ``e_cap - energy``."""
        cap = self._cap(e_cap)
        level = cap - float(energy)
        if not level > 0.0:
            raise ValueError("energy must lie below the cap (%r)" % cap)
        return density_components(self.capped(cap), self.cell, level, connectivity, ctx=ctx)

    def percolation(self, connectivity=26, e_cap=None, ctx=None):
        """The energies at which ``{E <= energy}`` first connects across the cell in one, two and three dimensions: the
        ``PercolationResult`` of the capped grid, with ``energies3`` - ``energies3[d - 1] = max{E[v] : g[v] >= t_d}``, the bytes of
        a voxel's energy, ``nan`` where the level is 0.0 - and ``barriers3 = energies3 - e_min``, the static migration barriers."""
        g = self.capped(e_cap)
        res = density_percolation(g, self.cell, connectivity, ctx=ctx)
        res.energies3 = level_energies(self.energies, g, res.levels)
        res.barriers3 = res.energies3 - self.e_min
        return res

    def voxel_of(self, points):
        """The voxel (flat index) of Cartesian points, by the rule of the density kernels."""
        return voxel_of(self.cell, self.grid, points)

    def match_sites(self, sn, window=None):
        """How the landscape and the sites of ``sn`` agree: a dict with ``site_energy`` (the energy at the voxel of every site
        centre), ``site_minimum`` and ``site_minimum_distance`` (the nearest minimum of every site and its minimum-image distance),
        ``minimum_site`` and ``minimum_site_distance`` (the nearest site of every minimum), ``minimum_voxels``,
        ``minimum_positions``, ``minimum_energies``."""
        centers = np.asarray(sn.centers, dtype=np.float64).reshape(-1, 3)
        with _lib.HipContext(self.cell) as ctx:                    # one context for the minima and the distances
            v, _, pos, e = self.minima(window, ctx=ctx)
            n_s, n_m = len(centers), len(v)
            dist = np.zeros((n_s, n_m))
            pbc = PBCCalculator(self.cell, _ctx=ctx)
            if n_m:
                for s in range(n_s):
                    dist[s] = pbc.distances(centers[s], pos)
        out = dict(site_energy=self.energies.reshape(-1)[self.voxel_of(centers)], minimum_voxels=v, minimum_positions=pos,
                   minimum_energies=e)
        if n_s and n_m:
            out["site_minimum"], out["site_minimum_distance"] = dist.argmin(axis=1), dist.min(axis=1)
            out["minimum_site"], out["minimum_site_distance"] = dist.argmin(axis=0), dist.min(axis=0)
        else:
            out["site_minimum"], out["site_minimum_distance"] = np.full(n_s, -1), np.full(n_s, np.inf)
            out["minimum_site"], out["minimum_site_distance"] = np.full(n_m, -1), np.full(n_m, np.inf)
        return out

    def write_cube(self, path, structure=None, e_cap=None):
        """A Gaussian cube file of the energies (units of ``epsilon``; ``+inf`` and everything above the cap written as ``e_cap``,
        by default the largest finite energy): the origin, the three voxel vectors - any cell shape - and the atoms of
        ``structure`` (``get_positions`` / ``get_atomic_numbers``), in bohr."""
        cap = self._cap(e_cap)
        g = np.minimum(self.energies, cap)
        steps = _voxel_vectors(self.cell, self.grid) / BOHR
        pos = np.zeros((0, 3)) if structure is None else np.asarray(structure.get_positions(), dtype=np.float64) / BOHR
        numbers = np.zeros(0, dtype=np.int64) if structure is None else np.asarray(structure.get_atomic_numbers())
        with open(path, "w") as fh:
            fh.write("probe-ion energy (sitator_amd.EnergyLandscape), units of epsilon\n")
            fh.write("capped at %.17e\n" % cap)
            origin = 0.5 * steps.sum(axis=0)                       # the value of a voxel stands at its centre
            fh.write("%5d %.17e %.17e %.17e\n" % ((len(pos),) + tuple(origin)))
            for a in range(3):
                fh.write("%5d %.17e %.17e %.17e\n" % ((self.grid[a],) + tuple(steps[a])))
            for z, p in zip(numbers, pos):
                fh.write("%5d %.6f %.17e %.17e %.17e\n" % (int(z), float(z), p[0], p[1], p[2]))
            for row in g.reshape(self.grid[0] * self.grid[1], self.grid[2]):
                for k in range(0, len(row), 6):
                    fh.write(" ".join("%.17e" % x for x in row[k:k + 6]) + "\n")


def level_energies(energies, capped, levels):
    """``[3]``: ``max{E[v] : g[v] >= t}`` for every level ``t`` of ``levels``, ``nan`` for a level of 0.0.  ``g`` is non-increasing
    in ``E``, so ``{g >= t}`` is a sublevel set of ``E`` and the value is the energy the set first connects at, as the bytes of a
    voxel's energy."""
    out = np.full(3, np.nan)
    for d, t in enumerate(np.asarray(levels, dtype=np.float64)):
        if t > 0.0:
            out[d] = energies[capped >= t].max()
    return out


class EnergyLandscape(object):
    """The energy of a probe ion on a grid over the cell, among the static atoms and all their periodic images.

    ``calculator``: a ``sitator_amd.calculators.LennardJones``.  ``grid``: a triple ``(n0, n1, n2)``, each in ``[1, 1024]``;
    without it ``n_a = ceil(|c_a| / spacing)``, clipped to that range (the rule of ``IonicDensity``).  ``form``: 0 lets the library
    choose between its kernels, 1 and 2 force the direct and the tiled one - the energies are the same bytes."""

    def __init__(self, calculator, grid=None, spacing=0.2, form=0):
        if not isinstance(calculator, LennardJones):
            raise TypeError("EnergyLandscape: `calculator` must be a sitator_amd.calculators.LennardJones, not %s: the energies are "
                            "evaluated on the device and there is no CPU fallback" % type(calculator).__name__)
        self.calculator = calculator
        self.grid = None if grid is None else tuple(int(v) for v in np.asarray(grid).reshape(3))
        self.spacing, self.form = float(spacing), int(form)
        if self.grid is None and not self.spacing > 0:
            raise ValueError("spacing must be positive")

    def grid_for(self, cell):
        if self.grid is not None:
            return self.grid
        lengths = np.linalg.norm(np.asarray(cell, dtype=np.float64), axis=1)
        return tuple(int(v) for v in np.clip(np.ceil(lengths / self.spacing), 1, MAX_GRID))

    def compute_for_positions(self, static_pos, numbers, cell, ctx=None):
        """``static_pos`` ``[S, 3]``: the atoms of the frozen lattice, ``numbers`` ``[S]`` their atomic numbers, ``cell``: rows are
        the cell vectors.  ``ctx``: a ``HipContext`` of that cell to run on; without it one is made for the call.  Returns a
        ``LandscapeResult``."""
        from . import _lib_landscape
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        eps, sigma = self.calculator.parameters_for(numbers)
        energies, info = _with_ctx(cell, ctx, lambda c: _lib_landscape.landscape_energies(
            c, static_pos, eps, sigma, self.calculator.rc, self.grid_for(cell), self.form))
        return LandscapeResult(energies, cell, info)

    def compute(self, sn, ctx=None):
        """The landscape of the static atoms of the ``SiteNetwork`` ``sn`` under its structure's cell."""
        mask = sn.static_mask
        return self.compute_for_positions(np.asarray(sn.structure.get_positions(), dtype=np.float64)[mask],
                                          np.asarray(sn.structure.get_atomic_numbers())[mask], sn.structure.cell, ctx=ctx)
