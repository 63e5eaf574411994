"""``IonicDensity``: the time-averaged probability density of the mobile ions on a real-space grid over the cell (no
counterpart in the reference; ``DESIGN.md`` section 23) - what is shown as an isosurface beside a site analysis, and what the
sites are judged by: do the maxima of the density lie on the site centres, and where are the ions while they are unassigned.

The counts come from HIP kernels (``sit_density``, bound in ``_lib_density.py``) as integers per voxel - the same bytes on every
call - also straight from the trajectory a ``LandmarkAnalysis`` left resident, and split by the class of the site an ion is assigned
to where the labels of a ``SiteTrajectory`` are given.  A Gaussian smoothing is a list of taps whose weights are made here, on the
host; the device adds them up in list order.  The peaks of a grid come from the device too (``sit_density_peaks``)."""
import numpy as np

from . import _lib
from .dynamics import _resident_columns, _selected_columns
from .pbc import PBCCalculator
from .site_trajectory import SiteTrajectory

MAX_GRID = 1024
MAX_TAPS = 1 << 15
BOHR = 0.52917721067        # Angstrom: a cube file is written in atomic units


def _voxel_vectors(cell, grid):
    return np.asarray(cell, dtype=np.float64) / np.asarray(grid, dtype=np.float64)[:, None]


def gaussian_stencil(cell, grid, sigma, cutoff=4.0):
    """``(taps int64 [n, 3], weights float64 [n])``: every integer offset ``d`` of the grid whose Cartesian length
    ``|d0 c0 / n0 + d1 c1 / n1 + d2 c2 / n2|`` is at most ``cutoff * sigma``, in lexicographic order, with the weights
    ``exp(-r^2 / 2 sigma^2)`` divided by their sum.  ``ValueError`` where an offset would reach ``|d_a| > (n_a - 1) // 2`` (the
    stencil would meet its own periodic image) or where there are more than 2^15 taps."""
    grid = np.asarray(grid, dtype=np.int64).reshape(3)
    if not sigma > 0 or not cutoff > 0:
        raise ValueError("sigma and cutoff must be positive")
    steps = _voxel_vectors(cell, grid)
    r_max = float(cutoff) * float(sigma)
    # an offset of length <= r_max has |d_a| <= r_max / (distance between the lattice planes of the voxel lattice along a)
    heights = 1.0 / np.linalg.norm(np.linalg.inv(steps), axis=0)
    reach = np.floor(r_max / heights).astype(np.int64) + 1
    if np.prod(2.0 * reach + 1.0) > 5e7:
        raise ValueError("more than 2^15 taps: a smaller sigma or a coarser grid is needed")
    axes = [np.arange(-m, m + 1, dtype=np.int64) for m in reach]
    d = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)         # lexicographic
    vec = d.astype(np.float64) @ steps
    r2 = np.einsum("ij,ij->i", vec, vec)
    keep = np.sqrt(r2) <= r_max
    taps, r2 = np.ascontiguousarray(d[keep]), r2[keep]
    if len(taps) > MAX_TAPS:
        raise ValueError("more than 2^15 taps: a smaller sigma or a coarser grid is needed")
    if np.any(np.abs(taps).max(axis=0) > (grid - 1) // 2):
        raise ValueError("the stencil reaches beyond (n - 1) // 2 voxels along an axis: a smaller sigma or a finer grid is needed")
    w = np.exp(-r2 / (2.0 * float(sigma) * float(sigma)))
    return taps, w / w.sum()


def voxel_of(cell, grid, points):
    """The voxel (flat index) of Cartesian points on the grid ``(n0, n1, n2)`` over ``cell``, by the rule of the kernels."""
    ci = np.linalg.inv(np.asarray(cell, dtype=np.float64).T)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    idx = []
    for a in range(3):
        s = (ci[a, 0] * p[:, 0] + ci[a, 1] * p[:, 1]) + ci[a, 2] * p[:, 2]
        i = ((s - np.floor(s)) * float(grid[a])).astype(np.int64)
        idx.append(np.where(i >= grid[a], grid[a] - 1, i))
    return (idx[0] * grid[1] + idx[1]) * grid[2] + idx[2]


class DensityResult(object):
    """What ``IonicDensity`` returns.  ``counts`` uint64 ``[n_classes, n0, n1, n2]`` as the device counted them; ``n_frames``, the
    frames taken; ``skipped``, the entries with a coordinate that is not finite; ``voxel_volume`` in A^3; ``density`` =
    ``counts / (n_frames * voxel_volume)``, ions per A^3; ``smoothed``: the counts under the taps, float64 of the same shape, or
    ``None``; ``class_names``, one per plane; ``cell``, ``grid``."""

    def __init__(self, counts, n_frames, skipped, cell, smoothed, class_names):
        self.counts, self.n_frames, self.skipped, self.smoothed = counts, int(n_frames), int(skipped), smoothed
        self.cell = np.asarray(cell, dtype=np.float64)
        self.grid = tuple(int(v) for v in counts.shape[1:])
        self.class_names = tuple(class_names)
        self.voxel_volume = abs(float(np.linalg.det(self.cell))) / float(np.prod(self.grid))

    @property
    def density(self):
        """Ions per A^3: made when asked for (a grid of 0.2 A voxels holds millions of them)."""
        return self.counts.astype(np.float64) / (float(self.n_frames) * self.voxel_volume)

    def fractional_centers(self):
        """``[n0, n1, n2, 3]``: the fractional coordinates of the voxel centres."""
        axes = [(np.arange(n) + 0.5) / n for n in self.grid]
        return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)

    def cartesian_centers(self):
        return self.fractional_centers() @ self.cell

    def _plane(self, plane, smoothed=True):
        """The grid of one plane, or (``None``) the sum of the planes: the smoothed counts where there are any."""
        src = self.smoothed if (smoothed and self.smoothed is not None) else self.counts.astype(np.float64)
        return src.sum(axis=0) if plane is None else np.ascontiguousarray(src[plane])

    def free_energy(self, kT, plane=None):
        """``-kT ln(rho / rho_max)`` of the smoothed grid if there is one, else the raw one; ``inf`` where it is 0."""
        g = self._plane(plane)
        top = g.max()
        with np.errstate(divide="ignore", invalid="ignore"):
            out = -float(kT) * np.log(g / top)
        out[g == top] = 0.0
        out[g <= 0.0] = np.inf                                     # also an all-empty grid: nowhere is a maximum
        return out

    def peaks(self, min_fraction=0.05, plane=None, ctx=None):
        """``(voxels int64 [n], fractional [n, 3], cartesian [n, 3], values [n])``: the voxels whose value is at least
        ``min_fraction`` of the largest and exceeds that of their 26 periodic neighbours (equal values: the lowest index wins), found
        on the device, sorted by value descending with ties by index.  ``ctx``: a ``HipContext`` to run on (any: the peak rule
        does not look at its cell); without it one is made for the call."""
        from . import _lib_density
        g = self._plane(plane)
        threshold = float(min_fraction) * float(g.max())
        if ctx is not None:
            v = _lib_density.density_peaks(ctx, g, threshold)
        else:
            with _lib.HipContext(self.cell) as own:
                v = _lib_density.density_peaks(own, g, threshold)
        values = g.reshape(-1)[v]
        order = np.lexsort((v, -values))
        v, values = v[order], values[order]
        fr = self.fractional_centers().reshape(-1, 3)[v]
        return v, fr, fr @ self.cell, values

    def components(self, level, connectivity=26, plane=None, ctx=None):
        """The connected components of ``{g >= level}`` of the smoothed grid if there is one, else the raw one, with the rank and the
        basis of every component's loop lattice: a ``ComponentsResult`` (``percolation.py``)."""
        from .percolation import density_components
        return density_components(self._plane(plane), self.cell, level, connectivity, ctx=ctx)

    def percolation(self, connectivity=26, plane=None, ctx=None):
        """The levels at which that grid first connects across the cell in one, two and three dimensions: a ``PercolationResult``."""
        from .percolation import density_percolation
        return density_percolation(self._plane(plane), self.cell, connectivity, ctx=ctx)

    def voxel_of(self, points):
        """The voxel (flat index) of Cartesian points, by the rule of the kernels."""
        return voxel_of(self.cell, self.grid, points)

    def match_sites(self, sn, min_fraction=0.05, plane=None):
        """How the density and the sites of ``sn`` agree: a dict with ``site_density`` (the density at the voxel of every site
        centre, ions per A^3), ``site_peak`` and ``site_peak_distance`` (the nearest peak of every site and its minimum-image
        distance), ``peak_site`` and ``peak_site_distance`` (the nearest site of every peak), ``peak_voxels``, ``peak_positions``."""
        centers = np.asarray(sn.centers, dtype=np.float64).reshape(-1, 3)
        with _lib.HipContext(self.cell) as ctx:                    # one context for the peaks and the distances
            v, _, pos, _ = self.peaks(min_fraction, plane, ctx=ctx)
            n_s, n_p = len(centers), len(v)
            dist = np.zeros((n_s, n_p))
            pbc = PBCCalculator(self.cell, _ctx=ctx)
            if n_p:
                for s in range(n_s):
                    dist[s] = pbc.distances(centers[s], pos)
        dens = (self.density.sum(axis=0) if plane is None else self.density[plane]).reshape(-1)
        out = dict(site_density=dens[self.voxel_of(centers)], peak_voxels=v, peak_positions=pos)
        if n_s and n_p:
            out["site_peak"], out["site_peak_distance"] = dist.argmin(axis=1), dist.min(axis=1)
            out["peak_site"], out["peak_site_distance"] = dist.argmin(axis=0), dist.min(axis=0)
        else:
            out["site_peak"], out["site_peak_distance"] = np.full(n_s, -1), np.full(n_s, np.inf)
            out["peak_site"], out["peak_site_distance"] = np.full(n_p, -1), np.full(n_p, np.inf)
        return out

    def write_cube(self, path, structure=None, plane=None):
        """A Gaussian cube file of the density (ions per bohr^3, from the smoothed counts if there are any): the origin, the three
        voxel vectors - any cell shape - and the atoms of ``structure`` (``get_positions`` / ``get_atomic_numbers``), in bohr."""
        g = self._plane(plane) / (float(self.n_frames) * self.voxel_volume) * BOHR ** 3
        steps = _voxel_vectors(self.cell, self.grid) / BOHR
        pos = np.zeros((0, 3)) if structure is None else np.asarray(structure.get_positions(), dtype=np.float64) / BOHR
        numbers = np.zeros(0, dtype=np.int64) if structure is None else np.asarray(structure.get_atomic_numbers())
        with open(path, "w") as fh:
            fh.write("ionic density (sitator_amd.IonicDensity), ions per bohr^3\n")
            fh.write("planes: %s\n" % ("all" if plane is None else self.class_names[plane]))
            # the value of a voxel stands at its centre
            origin = 0.5 * steps.sum(axis=0)
            fh.write("%5d %.17e %.17e %.17e\n" % ((len(pos),) + tuple(origin)))
            for a in range(3):
                fh.write("%5d %.17e %.17e %.17e\n" % ((self.grid[a],) + tuple(steps[a])))
            for z, p in zip(numbers, pos):
                fh.write("%5d %.6f %.17e %.17e %.17e\n" % (int(z), float(z), p[0], p[1], p[2]))
            flat = g.reshape(self.grid[0] * self.grid[1], self.grid[2])
            for row in flat:
                for k in range(0, len(row), 6):
                    fh.write(" ".join("%.17e" % x for x in row[k:k + 6]) + "\n")


class IonicDensity(object):
    """The probability density of chosen atoms on a grid over the cell, averaged over every ``frame_stride``-th frame.

    ``grid``: a triple ``(n0, n1, n2)``, each in ``[1, 1024]``; without it ``n_a = ceil(|c_a| / spacing)``, clipped to that range.
    ``sigma`` (A): a Gaussian smoothing of the counts over the offsets within ``cutoff * sigma`` (``gaussian_stencil``); ``None``:
    none.  ``form``: 0 lets the library choose how a workgroup adds up its counts, 1 and 2 force the direct and the aggregated
    form - the counts are the same bytes.  A point is put into the voxel ``floor(f n)`` of its fractional coordinate ``f`` reduced
    to ``[0, 1)``, so the trajectory is read as it is, wrapped or not; an atom with a coordinate that is not finite is counted in
    ``skipped``."""

    def __init__(self, grid=None, spacing=0.2, sigma=None, cutoff=4.0, frame_stride=1, form=0, workspace_bytes=0):
        self.grid = None if grid is None else tuple(int(v) for v in np.asarray(grid).reshape(3))
        self.spacing, self.sigma, self.cutoff = float(spacing), sigma, float(cutoff)
        self.frame_stride, self.form, self.workspace_bytes = int(frame_stride), int(form), int(workspace_bytes)
        if self.grid is None and not self.spacing > 0:
            raise ValueError("spacing must be positive")
        if self.frame_stride < 1:
            raise ValueError("frame_stride must be at least 1")

    def grid_for(self, cell):
        if self.grid is not None:
            return self.grid
        lengths = np.linalg.norm(np.asarray(cell, dtype=np.float64), axis=1)
        return tuple(int(v) for v in np.clip(np.ceil(lengths / self.spacing), 1, MAX_GRID))

    def _run(self, ctx, atoms, positions=None, site_class=None, class_names=("all",)):
        from . import _lib_density
        if len(atoms) == 0:
            raise ValueError("The selection holds no atom")
        grid = self.grid_for(ctx.cell)
        taps = weights = None
        if self.sigma is not None:
            taps, weights = gaussian_stencil(ctx.cell, grid, self.sigma, self.cutoff)
        counts, smoothed, taken, skipped = _lib_density.density(
            ctx, atoms, grid, positions=positions, frame_stride=self.frame_stride, site_class=site_class, n_classes=len(class_names),
            taps=taps, weights=weights, form=self.form, workspace_bytes=self.workspace_bytes)
        return DensityResult(counts, taken, skipped, ctx.cell, smoothed, class_names)

    def compute(self, traj, cell, mask):
        """``traj``: a host trajectory ``[n_frames, n_atoms, 3]``, float64, not modified; ``cell``: rows are the cell vectors;
        ``mask``: the selection, a boolean mask or an index array.  Returns a ``DensityResult`` of one plane."""
        sel = _selected_columns(traj, mask)
        with _lib.HipContext(np.asarray(cell, dtype=np.float64)) as ctx:
            return self._run(ctx, np.arange(sel.shape[1], dtype=np.int64), positions=sel)

    def compute_for_analysis(self, la, mask=None):
        """The same from the trajectory a ``LandmarkAnalysis`` that has run left on its GPU, under that analysis' cell: no upload.
        ``mask=None``: the mobile atoms of the run.  ``NotImplementedError`` after a run over frame shards."""
        ctx, atoms = _resident_columns(la, mask, "IonicDensity")
        return self._run(ctx, atoms)

    def compute_for_trajectory(self, la, st=None, classes="assigned"):
        """The density of the mobile atoms from the resident frames of ``la``, split into planes by the site every ion is assigned
        to at every frame - the labels of ``st`` (``None``: the trajectory ``la.run()`` returned; otherwise one that shares the
        analysis' device context, whose labels are brought up to date on the device first).  ``classes``: ``"assigned"`` - two
        planes, assigned and unassigned; ``"site_types"`` - one plane per value of ``sn.site_types`` in ascending order, then the
        unassigned one; an int array ``[n_sites]`` of classes ``0 .. C - 1`` - ``C`` planes and the unassigned one.  The planes add
        up to what ``compute_for_analysis(la)`` gives."""
        ctx, atoms = _resident_columns(la, None, "IonicDensity")
        if la._recenter_masses is not None:
            raise ValueError("The analysis recentred its frames on the device (recenter_masses): they are not the "
                             "trajectory run() was given")
        if st is None:
            ref = getattr(la, "_result", None)
            st = ref() if ref is not None else None
            if st is None:
                raise ValueError("The trajectory this analysis returned does not exist any more; pass `st`")
        assert isinstance(st, SiteTrajectory)
        if st._ctx is not la._ctx:
            raise ValueError("`st` does not share the device context of this analysis")
        sn = st.site_network
        n_sites = sn.n_sites
        if n_sites < 1:
            raise ValueError("The site network holds no site")
        if isinstance(classes, str):
            if classes == "assigned":
                site_class, names = np.zeros(n_sites, dtype=np.int32), ("assigned", "unassigned")
            elif classes == "site_types":
                if sn.site_types is None:
                    raise ValueError("The site network has no site types")
                types, site_class = np.unique(np.asarray(sn.site_types), return_inverse=True)
                names = tuple("type %s" % t for t in types) + ("unassigned",)
            else:
                raise ValueError("classes is \"assigned\", \"site_types\" or an int array over the sites")
        else:
            site_class = np.asarray(classes)
            if site_class.shape != (n_sites,) or site_class.dtype.kind not in "iu" or site_class.min() < 0:
                raise ValueError("classes must hold one class >= 0 per site")
            names = tuple("class %d" % k for k in range(int(site_class.max()) + 1)) + ("unassigned",)
        if len(names) > 16:
            raise ValueError("At most 15 classes beside the unassigned one")
        ctx = st._device()
        return self._run(ctx, atoms, site_class=np.ascontiguousarray(site_class, dtype=np.int32), class_names=names)
