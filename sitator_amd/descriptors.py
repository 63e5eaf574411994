"""``ConfigurationalEntropy`` (reference: ``sitator/descriptors/ConfigurationalEntropy.py``): the S~ configurational entropy of a
``SiteTrajectory``, a scalar statistic of the residences ``JumpAnalysis`` leaves on the site network.  Host numpy."""
import logging

import numpy as np

from .dynamics import JumpAnalysis
from .site_trajectory import SiteTrajectory

logger = logging.getLogger(__name__)


class ConfigurationalEntropy(object):
    """The S~ (S tilde) configurational entropy of Kweon et al., Chem. Mater. 2017, 29 (21), 9142-9153
    (DOI 10.1021/acs.chemmater.7b02902).

    With site types on the network (``SiteTypeAnalysis``, ``SiteCoordinationEnvironment``) the sum runs over the types, otherwise
    over the sites.  ``acceptable_overshoot``: an occupation probability above 1 by less than this is taken as 1; any other one
    above 1 raises ``ValueError``."""

    def __init__(self, acceptable_overshoot=0.0):
        self.acceptable_overshoot = acceptable_overshoot

    def compute(self, st):
        """S~ of ``st``.  Runs ``JumpAnalysis`` when the network lacks ``total_corrected_residences``; ``NotImplementedError`` on
        a frame shard."""
        assert isinstance(st, SiteTrajectory)
        if st._comm is not None and st._comm.size > 1:
            raise NotImplementedError("ConfigurationalEntropy needs all frames of the trajectory on one GPU; this trajectory is "
                                      "a frame shard")
        sn = st.site_network
        if not sn.has_attribute("total_corrected_residences"):
            JumpAnalysis().run(st)
        residences = np.asarray(sn.total_corrected_residences)
        if sn.site_types is not None:
            kinds = np.asarray(sn.site_types)
            _, N_i = np.unique(kinds, return_counts=True)
            n_i = np.empty(sn.n_types, dtype=np.float64)
            for i, kind in enumerate(sn.types):
                n_i[i] = np.true_divide(np.sum(residences[kinds == kind]), st.n_frames)
        else:
            N_i = np.ones(sn.n_sites)
            n_i = np.true_divide(residences, st.n_frames)
        p2 = np.true_divide(n_i, N_i)
        n = np.sum(n_i)
        problems = p2 > 1.0
        forgivable = problems & (p2 - 1.0 < self.acceptable_overshoot)
        logger.info("n_i      " + ("{:5.3} " * len(n_i)).format(*n_i))
        logger.info("N_i      " + ("{:>5} " * len(N_i)).format(*N_i))
        logger.info("P_2      " + ("{:5.3} " * len(p2)).format(*p2))
        if not np.all(problems == forgivable):
            raise ValueError("P_2 values for site types %s larger than 1.0 + acceptable_overshoot (%f)"
                             % (np.where(problems)[0], self.acceptable_overshoot))
        p2[forgivable] = 1.0
        return self.s_tilde(p2, n, N_i)

    def s_tilde(self, p2, n_occupied_sites, n_sites_of_type):
        """``- sum_i N_i (p_i ln p_i + (1 - p_i) ln(1 - p_i)) / n``; the terms with ``p_i`` of 0 or 1 are 0."""
        p2, n_sites_of_type = np.asarray(p2, dtype=np.float64), np.asarray(n_sites_of_type)
        nonzero = ~((p2 == 0.0) | (p2 == 1.0))
        p2 = p2[nonzero]
        inner = n_sites_of_type[nonzero] * (p2 * np.log(p2) + (1.0 - p2) * np.log(1.0 - p2))
        return -1.0 * np.sum(inner) / n_occupied_sites
