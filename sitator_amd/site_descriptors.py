"""Site descriptors.

``SOAP``, ``SOAPCenters``, ``SOAPSampledCenters``, ``SOAPDescriptorAverages`` (reference: ``sitator/site_descriptors/SOAP.py``) with
``device_soap_backend``: the power spectrum of DESIGN.md section 17, evaluated on the GPU (``sit_soap_vectors``,
``sit_soap_site_averages``).  The reference's QUIP and DScribe backends are not carried and there is no host fallback.

``SiteTypeAnalysis`` (reference: ``sitator/site_descriptors/SiteTypeAnalysis.py``): PCA of the descriptor vectors, density-peak
clustering of the projections and a vote per site, by the definitions of DESIGN.md section 18 (``sit_pca_covariance``,
``sit_pca_project``, ``sit_dpc_graph``, ``sit_dpc_assign``) instead of sklearn and pydpc.

``SiteCoordinationEnvironment`` (reference: ``sitator/site_descriptors/SiteCoordinationEnvironment.py``): the coordinating atoms of
every site and the continuous shape measure of their polyhedron by the definition of DESIGN.md section 19
(``sit_coordination_environments``) instead of pymatgen's ChemEnv.

``SiteVolumes`` (reference: ``sitator/site_descriptors/SiteVolumes.py``): the recentring of every site's point cloud runs on
the GPU for all sites at once (``sit_grouped_recenter_step``); the convex hulls are qhull's on the host (``hulls="host"``, the
default) or the device's (``hulls="device"``: ``sit_grouped_hull_volumes``, with qhull for the sites it flags)."""
import logging
import time

import numpy as np

from . import _lib
from .errors import CoordinationEnvironmentError
from .misc import resident_trajectory
from .site_network import SiteNetwork, Structure
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


# ---- SOAP --------------------------------------------------------------------------------------------------------------------

CHEMICAL_SYMBOLS = (
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd "
    "Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra "
    "Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
atomic_numbers = dict((sym, z + 1) for z, sym in enumerate(CHEMICAL_SYMBOLS))
assert len(CHEMICAL_SYMBOLS) == 118

SOAP_DEFAULTS = {"cutoff": 3.0, "l_max": 6, "n_max": 6, "atom_sigma": 0.4, "crossover": False, "cutoff_transition_width": 0.0}


def soap_radial_tables(cutoff, n_max, l_max):
    """``(alpha [l_max + 1, n_max], beta [l_max + 1, n_max, n_max])`` of the radial basis ``g_nl(r) = sum_n' beta[l][n][n'] r^l
    exp(-alpha[l][n'] r^2)``: ``r_n = linspace(1, cutoff, n_max)``, ``alpha = -ln(1e-3 / r_n^l) / r_n^2``, ``beta[l]`` the symmetric
    (Loewdin) inverse root of the overlap ``S = 0.5 Gamma(l + 3/2) (alpha_n + alpha_n')^-(l + 3/2)``."""
    from math import gamma
    rn = np.linspace(1.0, float(cutoff), int(n_max))
    alpha = np.empty((l_max + 1, n_max))
    beta = np.empty((l_max + 1, n_max, n_max))
    for l in range(l_max + 1):
        alpha[l] = -np.log(1e-3 / rn ** l) / rn ** 2
        overlap = 0.5 * gamma(l + 1.5) * (alpha[l][:, None] + alpha[l][None, :]) ** -(l + 1.5)
        w, v = np.linalg.eigh(overlap)
        beta[l] = (v / np.sqrt(w)) @ v.T
    return alpha, beta


def soap_n_dim(n_species, n_max, l_max, crossover):
    same, cross = n_max * (n_max + 1) // 2 * (l_max + 1), n_max * n_max * (l_max + 1)
    return n_species * same + (n_species * (n_species - 1) // 2 * cross if crossover else 0)


def soap_tables(n_species, soap_params={}):
    """The dict ``HipContext.soap_vectors`` takes: the parameters (``SOAP_DEFAULTS`` updated with ``soap_params``), the radial
    tables and ``n_dim``."""
    unknown = set(soap_params) - set(SOAP_DEFAULTS)
    if unknown:
        raise ValueError("Unknown SOAP parameters %r; the device backend knows %r" % (sorted(unknown), sorted(SOAP_DEFAULTS)))
    soap = dict(SOAP_DEFAULTS)
    soap.update(soap_params)
    soap["l_max"], soap["n_max"], soap["n_species"] = int(soap["l_max"]), int(soap["n_max"]), int(n_species)
    if soap["n_max"] < 1 or soap["l_max"] < 0 or not soap["cutoff"] > 0:
        raise ValueError("SOAP needs n_max >= 1, l_max >= 0 and a positive cutoff")
    soap["alpha"], soap["beta"] = soap_radial_tables(soap["cutoff"], soap["n_max"], soap["l_max"])
    soap["n_dim"] = soap_n_dim(soap["n_species"], soap["n_max"], soap["l_max"], bool(soap["crossover"]))
    return soap


class _DeviceSoaper(object):
    """What ``device_soap_backend`` hands to the operators: ``soaper(structure, positions)`` -> SOAP vectors, with ``n_dim``."""

    def __init__(self, sn, soap_mask, tracer_atomic_number, environment_list, soap_params):
        self.environment_list = [int(z) for z in environment_list]
        self.soap = soap_tables(len(self.environment_list), soap_params)
        self.n_dim = self.soap["n_dim"]
        self.cell = np.asarray(sn.structure.cell, dtype=np.float64)

    def species_idx(self, numbers):
        """The index of every atom's species in the environment list, -1 for an atom outside it."""
        idx = np.full(len(numbers), -1, dtype=np.int32)
        for k, z in enumerate(self.environment_list):
            idx[np.asarray(numbers) == z] = k
        return idx

    def __call__(self, structure, positions, ctx=None):
        own = ctx is None
        if own:
            ctx = _lib.HipContext(self.cell)
        try:
            out, _ = ctx.soap_vectors(structure.positions, self.species_idx(structure.get_atomic_numbers()), positions, self.soap)
        finally:
            if own:
                ctx.close()
        return out


def device_soap_backend(soap_params={}):
    """The backend of the SOAP operators: ``soap_params`` may set ``cutoff`` (3.0), ``l_max`` (6), ``n_max`` (6), ``atom_sigma``
    (0.4), ``crossover`` (False) and ``cutoff_transition_width`` (0: the hard cut)."""
    soap_params = dict(soap_params)
    soap_tables(1, soap_params)                                      # unknown keys and bad values fail here

    def backend(sn, soap_mask, tracer_atomic_number, environment_list):
        return _DeviceSoaper(sn, soap_mask, tracer_atomic_number, environment_list, soap_params)
    backend._device_soap_backend = True
    return backend


class SOAP(object):
    """Abstract base class for computing SOAP vectors in a ``SiteNetwork`` (``SOAP.py:13-147``).

    ``tracer_atomic_number``: the atomic number of the tracer (``None``: the first mobile atom's).  ``environment``: atomic
    numbers or symbols of the species to consider (``None``: every species the mask holds).  ``soap_mask``: which atoms of the
    structure form the host - a boolean mask, a tuple of symbols, or ``None`` for the static structure.  ``backend``: ``None`` or
    a ``device_soap_backend(...)``; anything else is a ``TypeError`` - the QUIP and DScribe backends are not carried."""

    def __init__(self, tracer_atomic_number, environment=None, soap_mask=None, backend=None):
        self.tracer_atomic_number = tracer_atomic_number
        self._soap_mask = soap_mask
        if backend is None:
            backend = device_soap_backend()
        if not getattr(backend, "_device_soap_backend", False):
            raise TypeError("`backend` must be a device_soap_backend(...): the QUIP and DScribe backends of the reference are not "
                            "carried, and there is no host fallback")
        self._backend = backend
        if environment is not None:
            if not isinstance(environment, (list, tuple)):
                raise TypeError('environment has to be a list or tuple of species (atomic number'
                                ' or symbol of the environment to consider')
            environment_list = []
            for e in environment:
                if isinstance(e, int):
                    assert 0 < e <= max(atomic_numbers.values())
                    environment_list.append(e)
                elif isinstance(e, str):
                    try:
                        environment_list.append(atomic_numbers[e])
                    except KeyError:
                        raise KeyError("You provided a string that is not a valid atomic symbol")
                else:
                    raise TypeError("Environment has to be a list of atomic numbers or atomic symbols")
            self._environment = environment_list
        else:
            self._environment = None

    def _prepare(self, stn):
        if isinstance(stn, SiteTrajectory):
            sn = stn.site_network
        elif isinstance(stn, SiteNetwork):
            sn = stn
        else:
            raise TypeError("`stn` must be SiteNetwork or SiteTrajectory")
        structure, tracer_atomic_number, soap_mask = self._make_structure(sn)
        if self._environment is not None:
            environment_list = self._environment
        else:
            environment_list = np.unique(sn.structure.get_atomic_numbers()[soap_mask])
        soaper = self._backend(sn, soap_mask, tracer_atomic_number, environment_list)
        return structure, tracer_atomic_number, soap_mask, soaper

    def get_descriptors(self, stn):
        """``(descs, desc_to_site)``: the descriptor vectors and, of equal length, the site each belongs to."""
        structure, tracer_atomic_number, soap_mask, soaper = self._prepare(stn)
        return self._get_descriptors(stn, structure, tracer_atomic_number, soap_mask, soaper)

    def _make_structure(self, sn):
        numbers = np.asarray(sn.structure.get_atomic_numbers())
        if self._soap_mask is None:
            soap_mask = sn.static_mask
        else:
            if isinstance(self._soap_mask, tuple):
                symbols = np.array([CHEMICAL_SYMBOLS[z - 1] if 0 < z <= 118 else "X" for z in numbers])
                soap_mask = np.isin(symbols, self._soap_mask)
            else:
                soap_mask = np.asarray(self._soap_mask, dtype=bool)
            assert not np.any(soap_mask & sn.mobile_mask), \
                "Error for atoms %s; No atom can be both static and mobile" % np.where(soap_mask & sn.mobile_mask)[0]
        assert np.any(soap_mask), "Given `soap_mask` excluded all host atoms."
        structure = Structure(np.asarray(sn.structure.positions, dtype=np.float64)[soap_mask], sn.structure.cell, numbers[soap_mask])
        if self._environment is not None:
            assert np.any(np.isin(numbers[soap_mask], self._environment)), \
                "Combination of given `soap_mask` with the given `environment` excludes all host atoms."
        if self.tracer_atomic_number is None:
            tracer_atomic_number = numbers[sn.mobile_mask][0]
        else:
            tracer_atomic_number = self.tracer_atomic_number
        if np.any(structure.get_atomic_numbers() == tracer_atomic_number):
            raise ValueError("Structure cannot have static atoms (that are enabled in the SOAP mask) of the same species as "
                             "`tracer_atomic_number`.")
        return structure, tracer_atomic_number, soap_mask

    def _get_descriptors(self, stn, structure, tracer_atomic_number, soap_mask, soaper):
        raise NotImplementedError


class SOAPCenters(SOAP):
    """The SOAPs of the site centres in the fixed host structure (``SOAP.py:152-166``)."""

    def _get_descriptors(self, sn, structure, tracer_atomic_number, soap_mask, soaper):
        if isinstance(sn, SiteTrajectory):
            sn = sn.site_network
        assert isinstance(sn, SiteNetwork), "SOAPCenters requires a SiteNetwork or SiteTrajectory, not `%s`" % sn
        return soaper(structure, sn.centers), np.arange(sn.n_sites)


class SOAPSampledCenters(SOAPCenters):
    """The SOAPs of representative points of every site, as ``sampling_transform`` makes them (``SOAP.py:169-192``):
    ``sitator_amd.misc.NAvgsPerSite`` for a ``SiteTrajectory``, ``sitator_amd.misc.GenerateAroundSites`` for a ``SiteNetwork``.  The
    transform must return a ``SiteNetwork`` whose ``site_types`` name the site a point was sampled from."""

    def __init__(self, *args, **kwargs):
        self.sampling_transform = kwargs.pop('sampling_transform', 1)
        super(SOAPSampledCenters, self).__init__(*args, **kwargs)

    def get_descriptors(self, stn):
        sampled = self.sampling_transform.run(stn)
        assert isinstance(sampled, SiteNetwork), "Sampling transform returned `%s`, not a SiteNetwork" % sampled
        dvecs, _ = super(SOAPSampledCenters, self).get_descriptors(sampled)
        return dvecs, sampled.site_types


class SOAPDescriptorAverages(SOAP):
    """Many instantaneous SOAPs per site, averaged in SOAP space (``SOAP.py:196-320``): one vector per assigned mobile ion per
    strided frame, in the host structure as it was at that moment, ``averaging`` of them to an output vector.

    ``stepsize``: stride in frames (1).  ``averaging``: vectors per output vector, or ``avg_descriptors_per_site``: the average
    number of output vectors per site.  All environments of a call are evaluated and added up on the GPU
    (``sit_soap_site_averages``); the vectors of an output row are added in ascending frame order, as the reference does."""

    def __init__(self, *args, **kwargs):
        averaging_key, stepsize_key, avg_desc_per_key = 'averaging', 'stepsize', 'avg_descriptors_per_site'
        assert not ((averaging_key in kwargs) and (avg_desc_per_key in kwargs)), \
            "`averaging` and `avg_descriptors_per_site` cannot be specified at the same time."
        self._stepsize = kwargs.pop(stepsize_key, 1)
        d = {stepsize_key: self._stepsize}
        if averaging_key in kwargs:
            self._averaging = kwargs.pop(averaging_key)
            d[averaging_key] = self._averaging
            self._avg_desc_per_site = None
        elif avg_desc_per_key in kwargs:
            self._avg_desc_per_site = kwargs.pop(avg_desc_per_key)
            d[avg_desc_per_key] = self._avg_desc_per_site
            self._averaging = None
        else:
            raise RuntimeError("Either the `averaging` or `avg_descriptors_per_site` option must be provided.")
        for k, v in d.items():
            if not isinstance(v, int):
                raise TypeError('{} has to be an integer'.format(k))
            if not (v > 0):
                raise ValueError('{} has to be an positive'.format(k))
        super(SOAPDescriptorAverages, self).__init__(*args, **kwargs)

    def get_descriptors(self, st):
        """From ``st.real_trajectory`` (host) and ``st``'s labels."""
        assert isinstance(st, SiteTrajectory), "SOAPDescriptorAverages requires a SiteTrajectory"
        if st.real_trajectory is None:
            raise ValueError("SiteTrajectory must have associated real trajectory.")
        real = np.asarray(st.real_trajectory)
        if real.dtype != np.float64:
            raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % real.dtype)
        return self._averages(st, real)

    def get_descriptors_for_analysis(self, la, st=None):
        """The same from the frames a ``LandmarkAnalysis`` that has run left on its GPU: no upload (guards as
        ``GenerateClampedTrajectory.run_for_analysis``; ``NotImplementedError`` after a run over frame shards)."""
        st = resident_trajectory(la, st, "SOAPDescriptorAverages.get_descriptors_for_analysis")
        return self._averages(st, None)

    def _averages(self, st, positions):
        if st._comm is not None and st._comm.size > 1:
            raise NotImplementedError("SOAPDescriptorAverages needs all frames of the trajectory on one GPU; this trajectory is a "
                                      "frame shard")
        sn = st.site_network
        structure, tracer_atomic_number, soap_mask, soaper = self._prepare(st)
        nsit = int(sn.n_sites)
        descs, counts, nr_of_descs, info = st._device().soap_site_averages(
            nsit, np.where(soap_mask)[0], soaper.species_idx(structure.get_atomic_numbers()), np.where(sn.mobile_mask)[0], soaper.soap,
            stepsize=self._stepsize, averaging=self._averaging, avg_descriptors_per_site=self._avg_desc_per_site, positions=positions)
        if info["averaging"] == 0:
            logger.warning("Asking for too many average descriptors per site; got averaging = 0; setting averaging = 1")
        averaging = max(info["averaging"], 1)
        logger.debug("Will average %i SOAP vectors for every output vector" % averaging)
        insufficient = counts // averaging == 0
        if np.any(insufficient):
            logger.warning("You're asking to average %i SOAP vectors, but at this stepsize, %i sites are insufficiently occupied. "
                           "Num occ./averaging: %s" % (averaging, np.sum(insufficient), counts[insufficient] / averaging))
        self.last_info = info
        return descs, np.repeat(np.arange(nsit), nr_of_descs)


# ---- SiteTypeAnalysis ----------------------------------------------------------------------------------------------------------

class DescriptorPCA(object):
    """What ``SiteTypeAnalysis`` keeps of its PCA, under sklearn's names: ``components_`` ``[d, D]``, ``explained_variance_``,
    ``explained_variance_ratio_`` (of the ``d`` components taken), ``mean_``, ``n_components_``."""

    def __init__(self, mean, components, explained_variance, explained_variance_ratio):
        self.mean_ = mean
        self.components_ = components
        self.explained_variance_ = explained_variance
        self.explained_variance_ratio_ = explained_variance_ratio
        self.n_components_ = len(components)


def pca_from_covariance(mean, cov, n_samples, min_pca_variance, min_pca_dimensions):
    """The host side of the PCA: sklearn's ``PCA(min_pca_variance)`` rule on the eigenvalues of ``cov`` (divisor
    ``n_samples - 1``) - ``n_components = searchsorted(cumsum(ratio), min_pca_variance, side="right") + 1`` over the
    ``min(n_samples, D)`` components a full SVD would give - and ``min_pca_dimensions`` components when fewer come out
    (``SiteTypeAnalysis.py:83-90``).  Column signs are ``numpy.linalg.eigh``'s: distances do not see them."""
    cov = np.asarray(cov, dtype=np.float64)
    D = cov.shape[0]
    w, v = np.linalg.eigh(cov)
    w, v = np.maximum(w[::-1], 0.0), v[:, ::-1]
    n_full = min(int(n_samples), D)
    w, v = w[:n_full], v[:, :n_full]
    ratio = w / np.sum(w)
    if not 0.0 < min_pca_variance < 1.0:
        raise ValueError("min_pca_variance must be in (0, 1), not %r" % (min_pca_variance,))
    n_components = int(np.searchsorted(np.cumsum(ratio), min_pca_variance, side="right")) + 1
    if n_components < min_pca_dimensions:
        logger.info("     PCA accounted for %.0f%% variance in only %i dimensions; less than minimum of %.0f."
                    % (100.0 * np.sum(ratio[:n_components]), n_components, min_pca_dimensions))
        logger.info("     Forcing PCA to use %i dimensions." % min_pca_dimensions)
        n_components = int(min_pca_dimensions)
    if not 1 <= n_components <= n_full:
        raise ValueError("n_components=%r must be between 1 and min(n_samples, n_features)=%r" % (n_components, n_full))
    return DescriptorPCA(np.asarray(mean, dtype=np.float64), np.ascontiguousarray(v[:, :n_components].T), w[:n_components],
                         ratio[:n_components])


class DensityPeaks(object):
    """Density-peak clustering of ``points`` ``[N, d]`` on the GPU (``sit_dpc_graph``, ``sit_dpc_assign``), under the attribute
    names of ``pydpc.Cluster``: ``kernel_size``, ``density``, ``delta``, ``neighbour``, ``order`` (densest first), and after
    ``assign(min_density, min_delta)`` ``clusters`` and ``membership``.  The definitions are those of ``csrc/dpc_plan.h``
    (DESIGN.md section 18); pydpc's halo and border are not carried."""

    def __init__(self, points, fraction=0.02, ctx=None):
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.npoints = len(self.points)
        self.fraction = fraction
        self._ctx = ctx
        self.kernel_size, self.density, self.delta, self.neighbour, self.info = ctx.dpc_graph(self.points, fraction)
        # densest first, equal densities by ascending index: the order `above` of the plan
        self.order = np.lexsort((np.arange(self.npoints), -self.density)).astype(np.int32)
        self.clusters = self.membership = self.votes = None

    def assign(self, min_density, min_delta, dvecs_to_site=None, n_sites=0):
        self.min_density, self.min_delta = min_density, min_delta
        self.membership, self.clusters, self.votes = self._ctx.dpc_assign(self.density, self.delta, self.neighbour, min_density,
                                                                          min_delta, dvecs_to_site, n_sites)
        self.nclusters = len(self.clusters)


class SiteTypeAnalysis(object):
    """Cluster sites into types using a continuous descriptor and Density Peak Clustering (``SiteTypeAnalysis.py``).

    Computes descriptor vectors, reduces them with a principal component analysis and clusters them with density-peak
    clustering; every site gets the type most of its descriptor vectors were assigned to.  The column statistics, the projection,
    the clustering and the vote run on the GPU (``sit_pca_covariance``, ``sit_pca_project``, ``sit_dpc_graph``,
    ``sit_dpc_assign``); there is no host fallback.

    ``descriptor``: anything with ``get_descriptors(st|sn)`` returning descriptor vectors ``(M, n_dim)`` and the site of each.
    ``min_pca_variance``: the proportion of the variance the taken components must explain.  ``min_pca_dimensions``: take at
    least this many.  ``n_site_types_max``: the largest number of clusters; must be reasonable for the automatic choice to work.
    The plot methods of the reference are not carried."""

    def __init__(self, descriptor, min_pca_variance=0.9, min_pca_dimensions=2, n_site_types_max=20):
        self.descriptor = descriptor
        self.min_pca_variance = min_pca_variance
        self.min_pca_dimensions = min_pca_dimensions
        self.n_site_types_max = n_site_types_max
        self._n_dvecs = None

    def run(self, descriptor_input, **kwargs):
        """``descriptor_input``: a ``SiteNetwork`` or ``SiteTrajectory``; returns a copy of the network with ``site_types``."""
        from .elbow import index_of_elbow
        if self._n_dvecs is not None:
            raise ValueError("Can't run SiteTypeAnalysis more than once!")
        logger.info(" -- Running SiteTypeAnalysis --")
        if isinstance(descriptor_input, SiteNetwork):
            sn = descriptor_input.copy()
        elif isinstance(descriptor_input, SiteTrajectory):
            if descriptor_input._comm is not None and descriptor_input._comm.size > 1:
                raise NotImplementedError("SiteTypeAnalysis needs the descriptors of the whole trajectory on one GPU; this "
                                          "trajectory is a frame shard")
            sn = descriptor_input.site_network.copy()
        else:
            raise RuntimeError("Input {}".format(type(descriptor_input)))

        logger.info("  - Computing Descriptor Vectors")
        self.dvecs, dvecs_to_site = self.descriptor.get_descriptors(descriptor_input, **kwargs)
        assert len(self.dvecs) == len(dvecs_to_site), "Length mismatch in descriptor return values"
        dvecs_to_site = np.asarray(dvecs_to_site, dtype=np.int64)
        assert np.min(dvecs_to_site) == 0 and np.max(dvecs_to_site) < sn.n_sites

        logger.info("  - Clustering Descriptor Vectors")
        ctx = _lib.HipContext(np.asarray(sn.structure.cell, dtype=np.float64))
        try:
            dvecs = np.ascontiguousarray(self.dvecs, dtype=np.float64)
            mean, cov = ctx.pca_covariance(dvecs)
            self.pca = pca_from_covariance(mean, cov, len(dvecs), self.min_pca_variance, self.min_pca_dimensions)
            self.dvecs = ctx.pca_project(dvecs, self.pca.mean_, self.pca.components_)
            logger.info("     Accounted for %.0f%% of variance in %i dimensions"
                        % (100.0 * np.sum(self.pca.explained_variance_ratio_), self.dvecs.shape[1]))

            self.dpc = DensityPeaks(self.dvecs, ctx=ctx)
            # the sorted density * delta plot (fig. 4 of the paper): its elbow is, more or less, the number of clusters
            decision_curve = self.dpc.density * self.dpc.delta
            decision_curve_sort = np.argsort(decision_curve)[::-1]
            decision_curve = decision_curve[decision_curve_sort[:int(self.n_site_types_max * 1.5)]]
            elbow = index_of_elbow(decision_curve)
            self._decision_curve = decision_curve
            self._decision_elbow = elbow
            if elbow == 0:
                raise ValueError("Something went wrong with the decision curve (elbow == 0); try more data.")
            # a little less than the minimum in both cases
            density_threshold = np.min(self.dpc.density[decision_curve_sort[:elbow]]) - 0.001
            delta_threshold = np.min(self.dpc.delta[decision_curve_sort[:elbow]]) - 0.001
            self._real_dpc_thresh = (density_threshold, delta_threshold)
            self.dpc.assign(density_threshold, delta_threshold, dvecs_to_site, sn.n_sites)
        finally:
            if getattr(self, "dpc", None) is not None:
                self.dpc._ctx = None                                 # the context goes; what was computed stays
            ctx.close()
        assignments = self.dpc.membership
        unassigned = assignments < 0
        self._n_unassigned = np.sum(unassigned)
        self._n_dvecs = len(self.dvecs)
        site_type_counts = np.bincount(assignments[~unassigned])
        self.n_types = len(self.dpc.clusters)
        assert self.n_types == len(site_type_counts), "Got %i types from the clustering, but counted %i" % (self.n_types,
                                                                                                          len(site_type_counts))
        logger.info("     Found %i site type clusters" % self.n_types)
        logger.info("     Failed to assign %i/%i descriptor vectors to clusters." % (self._n_unassigned, self._n_dvecs))

        # -- voting: votes[site, type] were counted on the device
        votes = self.dpc.votes
        n_votes = np.bincount(dvecs_to_site, minlength=sn.n_sites)
        types = np.empty(shape=sn.n_sites, dtype=np.int64)
        self.winning_vote_percentages = np.empty(shape=sn.n_sites, dtype=np.float64)
        for site in range(sn.n_sites):
            if votes is None or votes.shape[1] == 0 or not votes[site].any():
                raise ValueError("No votes for site %i; check clustering and descriptors." % site)
            winner = np.argmax(votes[site])
            self.winning_vote_percentages[site] = float(votes[site, winner]) / n_votes[site]
            types[site] = winner
        n_sites_of_each_type = np.bincount(types, minlength=self.n_types)
        sn.site_types = types
        logger.info(("             " + "Type {:<2} " * self.n_types).format(*range(self.n_types)))
        logger.info(("# of sites   " + "{:<8}" * self.n_types).format(*n_sites_of_each_type))
        if np.any(n_sites_of_each_type == 0):
            logger.warning("WARNING: Had site types with no sites; check clustering settings/voting!")
        return sn


class SiteCoordinationEnvironment(object):
    """Determine site types from local coordination environments.

    The reference moves one site atom through pymatgen's ChemEnv, one structure-environment computation per site.  Here every
    site is typed on the GPU by the self-contained definition of DESIGN.md section 19: the coordinating atoms are the face
    neighbours of the site's Voronoi cell among the static lattice (all periodic images) that pass ChemEnv's "simplest"
    distance and solid-angle cutoffs, and the environment is the library shape of that coordination number with the smallest
    continuous shape measure (Pinsky & Avnir), minimised over all vertex assignments.  Agreement with a pymatgen installation is
    not claimed.

    Adds the site attributes ``coordination_environments`` (``"T:4"``, ``"O:6"``, ...; ``"UN:<n>"`` when no library shape of
    that coordination number lies under ``max_csm``; ``"BAD:0"`` without a coordinating atom), ``site_type_confidences``,
    ``coordination_numbers`` and - beyond the reference - ``coordination_csm`` (the shape measure of the environment, NaN
    without one), and sets ``site_types`` and ``vertices`` (static indices, statics-only numbering, ordered by distance; an index
    repeats when two images of one atom coordinate the site, which only a tiny cell does).

    :param bool guess_ionic_bonds: ``True`` raises ``NotImplementedError``: bond-valence analysis is not carried.  The default
        is ``False``, where the reference's is ``True``.
    :param bool full_chemenv_site_types: number the site types by environment symbol (ascending) instead of by coordination
        number (ascending).  The reference's order is the hash order of a ``set`` and cannot be reproduced.
    :param float distance_cutoff: distance of a neighbour / smallest distance at most this (ChemEnv: 1.4).
    :param float angle_cutoff: solid angle of a neighbour's face / largest solid angle at least this (ChemEnv: 0.3).
    :param float max_csm: a shape is an environment only with a shape measure below this (ChemEnv: 8.0).
    :param float tolerance: ``tau`` in Angstrom of the certified empty-sphere tests.
    :param int device: the GPU.
    """

    def __init__(self, guess_ionic_bonds=False, full_chemenv_site_types=False, distance_cutoff=1.4, angle_cutoff=0.3, max_csm=8.0,
                 tolerance=1e-6, device=0):
        if guess_ionic_bonds:
            raise NotImplementedError("SiteCoordinationEnvironment: bond-valence analysis (guess_ionic_bonds) is not carried")
        if not tolerance > 0.0:
            raise ValueError("SiteCoordinationEnvironment: the tolerance must be positive")
        if not (distance_cutoff >= 1.0 and 0.0 < angle_cutoff <= 1.0 and max_csm > 0.0):
            raise ValueError("SiteCoordinationEnvironment: distance_cutoff >= 1, 0 < angle_cutoff <= 1 and max_csm > 0 are required")
        self._full_chemenv_site_types = bool(full_chemenv_site_types)
        self._distance_cutoff, self._angle_cutoff, self._max_csm = float(distance_cutoff), float(angle_cutoff), float(max_csm)
        self._tolerance = float(tolerance)
        self._device = int(device)
        self.last_info = None

    def run(self, sn):
        """``sn`` with type information.  Any site whose cell could not be certified raises ``CoordinationEnvironmentError``: a
        partly typed network is never returned."""
        assert isinstance(sn, SiteNetwork)
        if sn.n_sites == 0:
            logger.warning("Site network had no sites.")
            return sn
        static = sn.static_structure
        positions = np.ascontiguousarray(static.get_positions(), dtype=np.float64)
        cell = np.asarray(static.cell, dtype=np.float64).reshape(3, 3)
        ctx = _lib.HipContext(cell, device=self._device)
        try:
            res = ctx.coordination_environments(positions, sn.centers, self._tolerance, self._distance_cutoff, self._angle_cutoff,
                                                self._max_csm)
        finally:
            ctx.close()
        self.last_info = res["info"]
        bad = np.nonzero(res["status"] != 0)[0]
        if len(bad):
            raise CoordinationEnvironmentError(bad, res["status"][bad])
        near = np.nonzero(res["flags"] & 1)[0]
        if len(near):
            logger.warning("%d sites have a neighbour within 1e-9 (relative) of a cutoff: %s" % (len(near), near[:16].tolist()))
        numbers = res["n"].astype(np.int64)
        symbols = []
        for k in range(sn.n_sites):
            if numbers[k] == 0:
                symbols.append("BAD:0")
            elif res["shape"][k] >= 0:
                symbols.append(_lib.COORDENV_SHAPES[res["shape"][k]])
            else:
                symbols.append("UN:%d" % numbers[k])
        vertices = [[int(i) for i in v] for v in res["vertices"]]
        assert np.all(numbers == [len(v) for v in vertices])
        typearr = symbols if self._full_chemenv_site_types else [int(v) for v in numbers]
        unique_envs = sorted(set(typearr))
        site_types = np.array([unique_envs.index(t) for t in typearr])
        n_types = len(unique_envs)
        logger.info(("Type         " + "{:<8}" * n_types).format(*unique_envs))
        logger.info(("# of sites   " + "{:<8}" * n_types).format(*np.bincount(site_types)))
        csm = np.where(res["shape"] >= 0, res["csm_best"], np.nan)
        sn.site_types = site_types
        sn.vertices = vertices
        for name, value in (("coordination_environments", np.array(symbols)), ("site_type_confidences", res["confidence"].copy()),
                            ("coordination_numbers", numbers), ("coordination_csm", csm)):
            if sn.has_attribute(name):
                sn.remove_attribute(name)
            sn.add_site_attribute(name, value)
        return sn
