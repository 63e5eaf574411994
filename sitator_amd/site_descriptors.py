"""``SiteVolumes`` (reference: ``sitator/site_descriptors/SiteVolumes.py``): the recentring of every site's point cloud runs on
the GPU for all sites at once (``sit_grouped_recenter_step``); the convex hulls are qhull's on the host (``hulls="host"``, the
default) or the device's (``hulls="device"``: ``sit_grouped_hull_volumes``, with qhull for the sites it flags)."""
import logging
import time

import numpy as np

from .misc import resident_trajectory
from .site_network import SiteNetwork
from .site_trajectory import SiteTrajectory

logger = logging.getLogger(__name__)


class InsufficientCoordinatingAtomsError(Exception):
    pass


def _hull_tools():
    from scipy.spatial import ConvexHull
    try:
        from scipy.spatial import QhullError
    except ImportError:                                            # scipy < 1.8
        from scipy.spatial.qhull import QhullError
    return ConvexHull, QhullError


class SiteVolumes(object):
    """Volumes of sites.

    ``error_on_insufficient_coord``: ``compute_volumes`` needs at least 4 vertices per site; a site with fewer raises
    ``InsufficientCoordinatingAtomsError`` (``True``) or gets volume 0 and surface area NaN (``False``).

    ``hulls``: where ``compute_accessable_volumes`` takes its convex hulls.  ``"host"``: every recentred cloud comes back and
    goes through ``scipy.spatial.ConvexHull``, as in the reference.  ``"device"``: the clouds stay on the GPU and are wrapped
    there with a certified orientation test; a site the device does not close with certified signs (coplanar points, fewer
    than 4, more facets than its capacity) is fetched on its own and goes through the host branch, warning and ``inf`` rule
    included.  The device's volume of a closed hull differs from qhull's in the last digits.  After a
    call ``last_hull_status`` maps every device status (0 closed, 1 few points, 2 uncertain sign, 3 capacity, 4 not closed)
    to the number of hulls (sites x recentrings) that ended with it, and ``last_hull_times`` holds the seconds spent in the
    recentring kernels, the hull kernels, the fetches of flagged sites and their host hulls, and the largest facet count.
    ``compute_volumes`` always runs on the host."""

    HULLS = ("host", "device")

    def __init__(self, error_on_insufficient_coord=True, hulls="host"):
        if hulls not in self.HULLS:
            raise ValueError("hulls must be one of %r, not %r" % (self.HULLS, hulls))
        self.error_on_insufficient_coord = error_on_insufficient_coord
        self.hulls = hulls
        self.last_hull_status = None
        self.last_hull_times = None

    def compute_accessable_volumes(self, st, n_recenterings=8):
        """The volume of the convex hull around all positions assigned to a site: the minimum over ``n_recenterings``
        recentrings around ``n`` of its points (shift-and-wrap; a site that fills most of the cell gives bogus results, as
        in the reference).  Adds the site attribute ``accessable_site_volumes``.

        The points are grouped by site on the GPU; every recentring step shifts and wraps all sites' points there, in
        place and cumulatively as the reference does, and comes back as one array - bit-equal to the reference's, so the
        hulls (``scipy.spatial.ConvexHull``, on the host) are the reference's.  A hull qhull refuses is logged and skipped;
        if all of a site's are refused its volume is ``inf``.  A site without points raises ``IndexError``.  With
        ``hulls="device"`` nothing comes back but the volumes and the flagged sites (see the class)."""
        assert isinstance(st, SiteTrajectory)
        return self._accessible(st, st.group_real_positions(), n_recenterings)

    def compute_accessable_volumes_for_analysis(self, la, st=None, n_recenterings=8):
        """The same from the frames a ``LandmarkAnalysis`` that has run left on its GPU (guards as
        ``GenerateClampedTrajectory.run_for_analysis``)."""
        st = resident_trajectory(la, st, "SiteVolumes.compute_accessable_volumes_for_analysis")
        return self._accessible(st, st.group_real_positions(_resident=True), n_recenterings)

    def _accessible(self, st, grouping, n_recenterings):
        if self.hulls == "device":
            return self._accessible_device(st, grouping, n_recenterings)
        ConvexHull, QhullError = _hull_tools()
        K = grouping.n_sites
        offsets = grouping.offsets
        vols = np.full(K, np.inf)
        work = np.empty((int(offsets[-1]), 3))
        for i in range(int(n_recenterings)):
            grouping._ctx.grouped_recenter_step(i, n_recenterings, work)
            for site in range(K):
                try:
                    hull = ConvexHull(work[offsets[site]:offsets[site + 1]])
                except QhullError as qhe:
                    logger.warning("For site %i, iter %i: %s" % (site, i, qhe))
                    continue
                if hull.volume < vols[site]:
                    vols[site] = hull.volume
        st.site_network.add_site_attribute("accessable_site_volumes", vols)
        return vols

    def _accessible_device(self, st, grouping, n_recenterings):
        ConvexHull, QhullError = _hull_tools()
        ctx = grouping._ctx
        K = grouping.n_sites
        offsets = grouping.offsets
        vols = np.full(K, np.inf)
        counts = dict((k, 0) for k in range(5))
        times = {"recenter": 0.0, "hull": 0.0, "fetch": 0.0, "fallback": 0.0, "max_facets": 0}
        for i in range(int(n_recenterings)):
            ctx.grouped_recenter_step(i, n_recenterings, None)
            v, status, n_facets, _ = ctx.grouped_hull_volumes(K)
            info = ctx.group_info()
            times["recenter"] += 1e-3 * info["recenter_ms"]
            times["hull"] += 1e-3 * info["hull_ms"]
            if K:
                times["max_facets"] = max(times["max_facets"], int(n_facets.max()))
            for k, n in zip(*np.unique(status, return_counts=True)):
                counts[int(k)] = counts.get(int(k), 0) + int(n)
            closed = status == 0
            better = closed & (v < vols)
            vols[better] = v[better]
            for site in np.nonzero(~closed)[0]:
                t0 = time.perf_counter()
                pts = ctx.grouped_work_fetch(int(offsets[site]), int(offsets[site + 1] - offsets[site]))
                t1 = time.perf_counter()
                try:
                    hull = ConvexHull(pts)
                except QhullError as qhe:
                    logger.warning("For site %i, iter %i: %s" % (site, i, qhe))
                    hull = None
                if hull is not None and hull.volume < vols[site]:
                    vols[site] = hull.volume
                times["fetch"] += t1 - t0
                times["fallback"] += time.perf_counter() - t1
        self.last_hull_status = counts
        self.last_hull_times = times
        logger.info("device hulls by status: %r; %d of %d went to the host" % (counts, sum(counts.values()) - counts[0], sum(counts.values())))
        st.site_network.add_site_attribute("accessable_site_volumes", vols)
        return vols

    def compute_volumes(self, sn):
        """The volume and surface area of the convex hull of every site's static vertices: adds the site attributes
        ``site_volumes`` and ``site_surface_areas`` (NaN where qhull fails)."""
        from .pbc import PBCCalculator
        ConvexHull, QhullError = _hull_tools()
        assert isinstance(sn, SiteNetwork)
        if sn.vertices is None:
            raise ValueError("SiteNetwork must have verticies to compute volumes!")
        vols = np.empty(sn.n_sites)
        areas = np.empty(sn.n_sites)
        pbcc = PBCCalculator(sn.structure.cell)
        try:
            for site in range(sn.n_sites):
                pos = np.asarray(sn.static_structure.positions, dtype=np.float64)[list(sn.vertices[site])]
                if len(pos) < 4:
                    if self.error_on_insufficient_coord:
                        raise InsufficientCoordinatingAtomsError("Site %i had only %i vertices (less than needed 4)" % (site, len(pos)))
                    vols[site] = 0
                    areas[site] = np.nan
                    continue
                pos += pbcc.cell_centroid - sn.centers[site]
                pbcc.wrap_points(pos)
                try:
                    hull = ConvexHull(pos)
                    vols[site] = hull.volume
                    areas[site] = hull.area
                except QhullError:
                    logger.warning("Had QHull failure when computing volume of site %i" % site)
                    vols[site] = np.nan
                    areas[site] = np.nan
        finally:
            pbcc._ctx.close()
        sn.add_site_attribute("site_volumes", vols)
        sn.add_site_attribute("site_surface_areas", areas)

    def run(self, st):
        """For backwards compatibility."""
        self.compute_accessable_volumes(st)
