"""``GenerateAroundSites`` (reference: ``sitator/misc/GenerateAroundSites.py``) and ``NAvgsPerSite`` (reference: ``sitator/misc/NAvgsPerSite.py``) on the device-side grouping of the real positions by site
(``SiteTrajectory.group_real_positions``)."""
import numpy as np

from .site_network import SiteNetwork
from .site_trajectory import SiteTrajectory


def resident_trajectory(la, st, who):
    """The trajectory whose labels go with the frames ``la`` left on its GPU, with the guards of
    ``GenerateClampedTrajectory.run_for_analysis``: ``NotImplementedError`` after a run over frame shards, ``ValueError`` if
    the analysis recentred its frames on the device or ``st`` does not share its device context."""
    la._need_run()
    if getattr(la, "_children", None) is not None or la._comm.size > 1 or la._ctx is None:
        raise NotImplementedError("%s needs all frames of the trajectory on one GPU; this analysis ran over frame shards"
                                  % who)
    if la._recenter_masses is not None:
        raise ValueError("The analysis recentred its frames on the device (recenter_masses): they are not the "
                         "trajectory run() was given; use the variant that takes the trajectory's real_trajectory")
    if st is None:
        ref = getattr(la, "_result", None)
        st = ref() if ref is not None else None
        if st is None:
            raise ValueError("The trajectory this analysis returned does not exist any more; pass `st`")
    assert isinstance(st, SiteTrajectory)
    if st._ctx is not la._ctx:
        raise ValueError("`st` does not share the device context of this analysis; use the variant that takes `st` alone")
    return st


class NAvgsPerSite(object):
    """Given a ``SiteTrajectory``, a ``SiteNetwork`` with ``n`` average positions per site: average ``i`` of a site is
    ``PBCCalculator.average`` of its points ``i, i + n, i + 2 n, ...`` in trajectory order.  The ``site_types`` of the
    output are the index of the site that generated the average.

    ``error_on_insufficient``: a site with at most ``n`` points raises ``ValueError``; ``False``: its points themselves are
    taken.  ``weighted``: weight with the trajectory's confidences (the point of maximal confidence anchors the average).

    The points are grouped by site once on the GPU and every bucket is averaged there by one workgroup
    (``sit_grouped_bucket_averages``); the shifted and wrapped points are the reference's bit for bit, their sum is taken in
    a fixed order of its own, so a centre differs from the reference's by rounding only."""

    def __init__(self, n, error_on_insufficient=True, weighted=True):
        assert n % 2 == 0
        self.n = n
        self.error_on_insufficient = error_on_insufficient
        self.weighted = weighted

    def run(self, st):
        """``st.real_trajectory`` (host) grouped by ``st``'s labels.  Returns a ``SiteNetwork``."""
        assert isinstance(st, SiteTrajectory)
        if st.real_trajectory is None:
            raise ValueError("SiteTrajectory must have associated real trajectory.")
        return self._run(st, lambda: st.group_real_positions())

    def run_for_analysis(self, la, st=None):
        """The same from the frames a ``LandmarkAnalysis`` that has run left on its GPU: no upload.  ``st``: ``None`` (the
        trajectory ``la.run()`` returned) or one that shares the analysis' device context; guards as
        ``GenerateClampedTrajectory.run_for_analysis``."""
        st = resident_trajectory(la, st, "NAvgsPerSite.run_for_analysis")
        return self._run(st, lambda: st.group_real_positions(_resident=True))

    def _run(self, st, make_grouping):
        n, K = int(self.n), int(st.site_network.n_sites)
        if self.weighted and st.confidences is None and K > 0:
            raise ValueError("This SiteTrajectory has no confidences")
        grouping = make_grouping()
        counts = grouping.counts
        enough = counts > n
        if self.error_on_insufficient and not np.all(enough):
            site = int(np.argmin(enough))
            raise ValueError("Insufficient points assigned to site %i (%i) to take %i averages." % (site, counts[site], n))
        if K > 0 and np.any(enough):
            averages, _ = grouping._ctx.grouped_bucket_averages(K, n, self.weighted)
        parts = [averages[s] if enough[s] else grouping.positions(s) for s in range(K)]
        centers = np.concatenate(parts) if parts else np.zeros((0, 3))
        types = np.repeat(np.arange(K, dtype=np.int64), np.where(enough, n, counts)) if K else np.zeros(0, dtype=np.int64)
        sn = st.site_network.copy()
        sn.centers = centers
        sn.site_types = types
        assert not np.isnan(np.sum(sn.centers))
        return sn


class GenerateAroundSites(object):
    """``n`` normally distributed points (standard deviation ``sigma``) around every site: the sampling transform
    ``SOAPSampledCenters`` names for a ``SiteNetwork``.  The ``site_types`` of the output are the index of the site a point was
    generated from.  The numbers are drawn from ``np.random`` exactly as the reference draws them, so the same seed gives the same
    centres; they are wrapped into the cell with ``PBCCalculator.wrap_points``."""

    def __init__(self, n, sigma):
        self.n = n
        self.sigma = sigma

    def run(self, sn):
        from .pbc import PBCCalculator
        assert isinstance(sn, SiteNetwork)
        out = sn.copy()
        pbcc = PBCCalculator(sn.structure.cell)
        try:
            newcenters = np.asarray(sn.centers).repeat(self.n, axis=0)
            assert len(newcenters) == self.n * sn.n_sites
            newcenters += self.sigma * np.random.standard_normal(size=newcenters.shape)
            pbcc.wrap_points(newcenters)
        finally:
            pbcc._ctx.close()
        out.centers = newcenters
        out.site_types = np.repeat(np.arange(sn.n_sites), self.n)
        return out
