"""The analysis steps right after the landmark path, evaluated on the GPU over the
device-resident site assignments:

* ``JumpAnalysis``  (reference ``sitator/dynamics/JumpAnalysis.py:11-135``)
* ``SmoothSiteTrajectory``  (reference ``sitator/dynamics/SmoothSiteTrajectory.pyx:13-111``)
* ``MergeSitesByDynamics``  (reference ``sitator/dynamics/MergeSitesByDynamics.py:12-153``; host logic over the jump
  statistics, distances and averages through the device-backed ``PBCCalculator``)
* ``MergeSitesByThreshold``  (reference ``sitator/dynamics/MergeSitesByThreshold.py:11-87``; the co-occupancy matrix of
  ``forbid_multiple_occupancy`` comes from the device labels)
* ``RemoveUnoccupiedSites``  (reference ``sitator/dynamics/RemoveUnoccupiedSites.py:10-71``; the visit counts come from
  the device labels)
* ``ReplaceUnassignedPositions``  (reference ``sitator/dynamics/ReplaceUnassignedPositions.py:26-117``; the nearest known
  label before and after every unassigned frame comes from a two-directional scan of the device labels)
* ``AverageVibrationalFrequency``  (reference ``sitator/dynamics/AverageVibrationalFrequency.py:30-61``; speeds, their
  exact-length Fourier transform and the band average per atom on the device, also straight from the trajectory a
  ``LandmarkAnalysis`` left resident)
* ``GenerateClampedTrajectory``  (reference ``sitator/misc/GenerateClampedTrajectory.pyx:13-128``; one pass of the device
  over the resident labels and the frames, also straight from the trajectory a ``LandmarkAnalysis`` left resident)
* ``MeanSquaredDisplacement`` and ``diffusion_coefficient``  (no counterpart in the reference; the tracer and the collective
  mean squared displacement against the lag, unwrapped under the cell on the device, also straight from the trajectory a
  ``LandmarkAnalysis`` left resident)
* ``VanHoveCorrelation`` and ``RadialDistribution``  (no counterpart in the reference; the self and the distinct part of the
  van Hove function and ``g(r)`` as integer histograms of float64 minimum-image distances, also straight from the trajectory a
  ``LandmarkAnalysis`` left resident)
"""
import contextlib
import logging
import operator

import numpy as np

from . import _lib, errors

from .markov import markov_clustering
from .merging import MergeSites
from .pbc import PBCCalculator
from .site_trajectory import SiteTrajectory

logger = logging.getLogger(__name__)


class JumpAnalysis(object):
    """Jump statistics of a ``SiteTrajectory``.

    Adds to ``st.site_network`` the edge attributes ``n_ij`` (jumps i -> j), ``p_ij`` (probability of
    jumping to j being at i), ``jump_lag`` (mean frames spent at i before jumping to j, ``inf`` if never)
    and the site attributes ``residence_times``, ``occupancy_freqs``, ``total_corrected_residences``.
    """

    def __init__(self):
        pass

    def run(self, st):
        assert isinstance(st, SiteTrajectory)
        logger.info("Running JumpAnalysis...")
        sn = st.site_network
        n_sites = sn.n_sites
        # a label beyond n_sites (only an array the caller built or edited can hold one) is caught where the labels are
        # read anyway: the accumulation kernel checks what it indexes its K x K tables with and the call raises the
        # reference's IndexError (dynamics/JumpAnalysis.py:75-88) - no pass of the host over the 50-MB label array
        ctx = st._device()
        comm = st._comm
        n_frames = st.n_frames
        if comm is not None and comm.size > 1:
            # the per-ion state (last known site, time at it) flows from frame shard to frame shard
            last_in = tac_in = None
            parts = None
            for r in range(comm.size):
                failure = None
                if comm.rank == r:
                    try:
                        parts = ctx.jump_analysis(n_sites, last_in, tac_in)
                        halo = np.stack([parts[5], parts[6]])
                    except IndexError as e:
                        # (a label beyond the site tables on THIS rank: the others are about to wait for the halo - they
                        # get a flag instead and everybody raises)
                        failure = e
                        halo = np.full((2, sn.n_mobile), np.iinfo(np.int64).min, dtype=np.int64)
                else:
                    halo = np.zeros((2, sn.n_mobile), dtype=np.int64)
                halo = comm.bcast(halo, root=r)
                if sn.n_mobile > 0 and halo[1, 0] == np.iinfo(np.int64).min:
                    raise failure if failure is not None else IndexError(
                        "a site index beyond the %d sites of the network in the frames of rank %d" % (n_sites, r))
                if comm.rank == r + 1:
                    last_in, tac_in = halo[0], halo[1]
            n_ij = comm.allreduce_sum(parts[0])
            tsum = comm.allreduce_sum(parts[1])
            tn = comm.allreduce_sum(parts[2])
            total_time = comm.allreduce_sum(parts[3])
            n_problems = int(comm.allreduce_sum(np.array([parts[4]], dtype=np.int64))[0])
            n_frames = int(comm.allreduce_sum(np.array([n_frames], dtype=np.int64))[0])
        else:
            n_ij, tsum, tn, total_time, n_problems, _, _ = ctx.jump_analysis(n_sites)
        # the time before "jumping" to oneself is never recorded (JumpAnalysis.py:99)
        assert not np.any(np.nonzero(tsum.diagonal()))
        if n_problems != 0:
            logger.warning("Came across %i times where assignment and last known assignment were unassigned." % n_problems)
        jump_lag = np.full((n_sites, n_sites), np.inf)
        seen = tn > 0
        jump_lag[seen] = tsum[seen] / tn[seen]
        for name in ("n_ij", "p_ij", "jump_lag", "residence_times", "occupancy_freqs", "total_corrected_residences"):
            if sn.has_attribute(name):
                sn.remove_attribute(name)
        sn.add_edge_attribute("jump_lag", jump_lag)
        sn.add_edge_attribute("n_ij", n_ij)
        with np.errstate(divide="ignore", invalid="ignore"):
            sn.add_edge_attribute("p_ij", n_ij / total_time)
        res_times = np.empty(n_sites)
        for site in range(n_sites):
            finite = jump_lag[site] < np.inf
            res_times[site] = np.mean(jump_lag[site][finite]) if np.any(finite) else n_frames
        sn.add_site_attribute("residence_times", res_times)
        sn.add_site_attribute("occupancy_freqs", np.sum(n_ij, axis=0) / n_frames)
        sn.add_site_attribute("total_corrected_residences", total_time)
        return st


class SmoothSiteTrajectory(object):
    """Rolling-mode low-pass filter of every particle's site assignment.

    Args as the reference: ``window_threshold_factor`` (window width in units of the threshold),
    ``remove_unoccupied_sites``, ``set_unassigned_under_threshold``.  On a frame shard the ranks exchange the frames a
    window reaches over (``_run_on_shard``) and the result is the single-rank one, a shard again.
    """

    def __init__(self, window_threshold_factor=2.1, remove_unoccupied_sites=True, set_unassigned_under_threshold=True):
        self.window_threshold_factor = window_threshold_factor
        self.remove_unoccupied_sites = remove_unoccupied_sites
        self.set_unassigned_under_threshold = set_unassigned_under_threshold

    def run(self, st, threshold):
        window = self.window_threshold_factor * threshold
        wleft, wright = int(np.floor(window / 2)), int(np.ceil(window / 2))
        n_sites = int(st.site_network.n_sites)
        comm = st._comm
        if comm is not None and comm.size > 1:
            out, counts = self._run_on_shard(st, comm, wleft, wright, threshold, n_sites)
        else:
            res = st._device().running_mode(wleft, wright, threshold, self.set_unassigned_under_threshold, n_sites=n_sites)
            out, counts = res if n_sites > 0 else (res, np.zeros(0, dtype=np.int64))
        # a new trajectory around the smoothed labels (adopted, not copied: nothing else holds them), the confidences
        # shared as the reference's st.copy() shares them (SiteTrajectory.py:31-38 copies the assignments only)
        new = st._derive(st.site_network.copy(), out, st._confs)
        if self.remove_unoccupied_sites:
            # sites left without any assignment are dropped and the rest renumbered in order
            # (what the reference delegates to dynamics.RemoveUnoccupiedSites); which are left comes with the labels
            sn = new.site_network
            seen = counts > 0
            if not np.all(seen):
                n_new = int(np.sum(seen))
                if n_new < sn.n_mobile:                      # dynamics/RemoveUnoccupiedSites.py:42-47
                    raise errors.InsufficientSitesError(verb="Removing unoccupied sites", n_sites=n_new,
                                                        n_mobile=sn.n_mobile)
                trans = np.full(sn.n_sites + 1, -1, dtype=np.int64)
                trans[:-1][seen] = np.arange(n_new)
                new._traj = trans[out]
                verts, types = sn.vertices, sn.site_types
                newsn = sn.copy()
                newsn.centers = np.asarray(sn.centers)[seen]     # (the setter drops vertices and types)
                if verts is not None:
                    newsn.vertices = [v for v, keep in zip(verts, seen) if keep]
                if types is not None:
                    newsn.site_types = np.asarray(types)[seen]   # old_sn[seen_mask] keeps them (:62)
                new._sn = newsn
        new.site_network.clear_attributes()
        return new

    def _run_on_shard(self, st, comm, wleft, wright, threshold, n_sites):
        """``(smoothed labels, visit counts)`` of a frame shard as the single-rank run gives them: the labels of this
        rank's frames, the counts summed over the ranks.

        The window of a frame reaches ``wleft`` frames back and ``wright - 1`` frames ahead, so every rank needs that many
        frames of its neighbours.  One ``allgather`` carries every rank's frame count with its last ``wleft`` and first
        ``wright - 1`` frames (bands of fixed size, padded where a rank is shorter); a rank collects its halo from as many
        neighbours as it takes - a neighbour may hold fewer frames than the band, or none.  The mode runs on
        ``[before | own | after]`` in a scratch context, so windows are clipped only where the whole trajectory ends and the
        labels resident in the trajectory's own context (shared, perhaps, with the frames of a ``LandmarkAnalysis``) stay
        the shard's."""
        lab = np.ascontiguousarray(st._traj, dtype=np.int64)
        n, M = lab.shape
        nt, nh = wleft, max(wright - 1, 0)
        msg = np.full((nt + nh) * M + 1, SiteTrajectory.SITE_UNKNOWN, dtype=np.int64)
        msg[-1] = n
        bands = msg[:-1].reshape(nt + nh, M)
        tail, head = lab[n - min(n, nt):], lab[:min(n, nh)]
        bands[nt - len(tail):nt] = tail                         # the tail band ends with the rank's last frame
        bands[nt:nt + len(head)] = head                         # the head band starts with its first
        every = comm.allgather(msg)
        n_of = every[:, -1]
        bands_of = every[:, :-1].reshape(comm.size, nt + nh, M)
        before, after = [], []
        need = nt
        for r in range(comm.rank - 1, -1, -1):
            k = min(need, int(n_of[r]))
            before.insert(0, bands_of[r, nt - k:nt])
            need -= k
        need = nh
        for r in range(comm.rank + 1, comm.size):
            k = min(need, int(n_of[r]))
            after.append(bands_of[r, nt:nt + k])
            need -= k
        ext = np.concatenate(before + [lab] + after)
        nb = sum(len(b) for b in before)
        device = st._ctx.device if st._ctx is not None else None
        # closing(): the scratch context needs no more than close() of whatever class makes it
        cell = np.asarray(st.site_network.structure.cell, dtype=np.float64)
        with contextlib.closing(_lib.HipContext(cell, device=device)) as scratch:
            scratch.set_assignments(ext)
            res = scratch.running_mode(wleft, wright, threshold, self.set_unassigned_under_threshold, n_sites=n_sites)
        if n_sites == 0:
            return np.ascontiguousarray(res[nb:nb + n]), np.zeros(0, dtype=np.int64)
        out, counts = res
        # the counts came with the labels, the halo's included: those few frames are taken off again
        for halo in (out[:nb], out[nb + n:]):
            counts = counts - np.bincount(halo[halo >= 0], minlength=n_sites)
        return np.ascontiguousarray(out[nb:nb + n]), comm.allreduce_sum(counts)


class MergeSitesByDynamics(MergeSites):
    """Merges sites that exchange particles, by Markov clustering of a connectivity matrix from the jump statistics
    (reference ``dynamics/MergeSitesByDynamics.py``).

    ``distance_threshold``: connectivity between sites further apart than this (Angstrom) is zeroed;
    ``post_check_thresh_factor``: merged sites further apart than factor x threshold raise
    ``MergedSitesTooDistantError``; ``markov_parameters``: ``inflation`` / ``expansion`` / ``pruning_threshold`` for
    ``markov_clustering``.  The reference's constructor reads an undefined ``iterlimit`` (:54, a ``NameError`` there);
    here it is an ordinary keyword that, as in the reference's body, is stored and not used."""

    def __init__(self, connectivity_matrix_generator=None, distance_threshold=1.0, post_check_thresh_factor=1.5,
                 check_types=True, markov_parameters={}, iterlimit=100):
        super(MergeSitesByDynamics, self).__init__(
            maximum_merge_distance=post_check_thresh_factor * distance_threshold, check_types=check_types)
        if connectivity_matrix_generator is None:
            connectivity_matrix_generator = MergeSitesByDynamics.connectivity_n_ij
        assert callable(connectivity_matrix_generator)
        self.connectivity_matrix_generator = connectivity_matrix_generator
        self.distance_threshold = distance_threshold
        self.post_check_thresh_factor = post_check_thresh_factor
        self.check_types = check_types
        self.iterlimit = iterlimit
        self.markov_parameters = markov_parameters

    # -- connectivity matrix generators (:59-107)
    @staticmethod
    def connectivity_n_ij(sn):
        """``n_ij`` itself as connectivity."""
        return sn.n_ij

    @staticmethod
    def connectivity_jump_lag_biased(jump_lag_coeff=1.0, jump_lag_sigma=20.0, jump_lag_cutoff=np.inf,
                                     distance_coeff=0.5, distance_sigma=1.0):
        """``p_ij`` biased by Gaussians of the jump lag and of the distance between the sites (:69-107)."""
        def cfunc(sn):
            jl = np.array(sn.jump_lag, dtype=np.float64)
            jl -= 1.0                                   # the minimum lag is one frame
            jl /= jump_lag_sigma
            np.square(jl, out=jl)
            jl *= -0.5
            np.exp(jl, out=jl)                          # -inf -> 0
            jl[np.asarray(sn.jump_lag) > jump_lag_cutoff] = 0.
            pbccalc = PBCCalculator(np.asarray(sn.structure.cell, dtype=np.float64))
            dmat = pbccalc.pairwise_distances(np.asarray(sn.centers))
            dmat /= distance_sigma
            np.square(dmat, out=dmat)
            dmat *= -0.5
            np.exp(dmat, out=dmat)
            return (np.asarray(sn.p_ij) + jump_lag_coeff * jl) * (distance_coeff * dmat + (1 - distance_coeff))
        return cfunc

    def _get_sites_to_merge(self, st):
        sn = st.site_network
        if not sn.has_attribute("n_ij"):                # :113-115
            JumpAnalysis().run(st)
        pbcc = PBCCalculator(np.asarray(sn.structure.cell, dtype=np.float64))
        connectivity_matrix = np.array(self.connectivity_matrix_generator(sn), dtype=np.float64, copy=True)
        n_sites_before = sn.n_sites
        assert n_sites_before == connectivity_matrix.shape[0]
        centers_before = np.asarray(sn.centers)
        # diagnostic only (:127-146): strong fluxes over the distance cut-off are reported, not kept
        no_diag_graph = connectivity_matrix.astype(np.float64, copy=True)
        np.fill_diagonal(no_diag_graph, np.nan)
        with np.errstate(invalid="ignore"):
            edge_threshold = np.nanmean(no_diag_graph) + 3 * np.nanstd(no_diag_graph)
        n_alarming_ignored_edges = 0
        for i in range(n_sites_before):
            rest = centers_before[i + 1:]
            dists = pbcc.distances(centers_before[i], rest) if len(rest) else np.zeros(0)
            js_too_far = np.where(dists > self.distance_threshold)[0] + i + 1
            if np.any(connectivity_matrix[i, js_too_far] > edge_threshold) or \
               np.any(connectivity_matrix[js_too_far, i] > edge_threshold):
                n_alarming_ignored_edges += 1
            connectivity_matrix[i, js_too_far] = 0
            connectivity_matrix[js_too_far, i] = 0
        if n_alarming_ignored_edges > 0:
            logger.warning("  At least %i site pairs with high (z-score > 3) fluxes were over the given distance cutoff.\n"
                           "  This may or may not be a problem; but if `distance_threshold` is low, consider raising it."
                           % n_alarming_ignored_edges)
        return markov_clustering(connectivity_matrix, **self.markov_parameters)   # :153


class MergeSitesByThreshold(MergeSites):
    """Merges the connected components of the graph that a strict threshold on any edge attribute leaves (reference
    ``dynamics/MergeSitesByThreshold.py``).  The threshold is a keyword of ``run()``: ``run(st, threshold=0)``.

    ``attrname``: the edge attribute (``n_ij``, ``p_ij``, ``jump_lag``, ...); ``relation``: applied as
    ``relation(attribute, threshold)``; ``directed`` / ``connection``: passed to ``scipy.sparse.csgraph``'s
    ``connected_components``; ``distance_threshold``: sites further apart than this (Angstrom) are not connected;
    ``forbid_multiple_occupancy``: sites that were ever occupied in the same frame are not connected (the matrix of
    ``SiteTrajectory.compute_site_cooccupancy``, one pass of the device over the labels where the reference walks the
    frames); further keywords go to ``MergeSites``."""

    def __init__(self, attrname, relation=operator.ge, directed=True, connection='strong', distance_threshold=np.inf,
                 forbid_multiple_occupancy=False, **kwargs):
        self.attrname = attrname
        self.relation = relation
        self.directed = directed
        self.connection = connection
        self.distance_threshold = distance_threshold
        self.forbid_multiple_occupancy = forbid_multiple_occupancy
        super(MergeSitesByThreshold, self).__init__(**kwargs)

    def _get_sites_to_merge(self, st, threshold=0):
        from scipy.sparse.csgraph import connected_components
        sn = st.site_network
        n_sites = sn.n_sites
        attrmat = np.asarray(getattr(sn, self.attrname))
        assert attrmat.shape == (n_sites, n_sites), "`attrname` doesn't seem to indicate an edge property."
        connmat = np.array(self.relation(attrmat, threshold), copy=True)     # never the attribute itself (:50)
        if self.distance_threshold < np.inf:                                 # :53-62
            pbcc = PBCCalculator(np.asarray(sn.structure.cell, dtype=np.float64))
            centers = np.asarray(sn.centers)
            for i in range(n_sites - 1):
                js_too_far = np.where(pbcc.distances(centers[i], centers[i + 1:]) > self.distance_threshold)[0] + i + 1
                connmat[i, js_too_far] = False
                connmat[js_too_far, i] = False
        if self.forbid_multiple_occupancy:                                   # :64-70
            connmat[st.compute_site_cooccupancy()] = False
        np.fill_diagonal(connmat, True)                                      # :73
        n_merged_sites, labels = connected_components(connmat, directed=self.directed, connection=self.connection)
        return [np.where(labels == lbl)[0] for lbl in range(n_merged_sites)]


class RemoveUnoccupiedSites(object):
    """Drops the sites no particle is ever assigned to and renumbers the rest in order (reference
    ``dynamics/RemoveUnoccupiedSites.py``).  Which sites are visited is read from the device-resident labels
    (``sit_site_counts``; summed over the ranks on frame shards)."""

    def __init__(self):
        pass

    def run(self, st, return_kept_sites=False):
        """A ``SiteTrajectory`` over the visited sites: types, vertices, site and edge attributes of the kept sites
        are carried over (``old_sn[seen_mask]``, :60), the confidences are not, the real trajectory is.  With
        ``return_kept_sites``: ``(new_st, np.where(seen_mask))``.  When every site is visited ``st`` ITSELF is
        returned - alone, also with ``return_kept_sites=True``, as the reference does (:31-34)."""
        assert isinstance(st, SiteTrajectory)
        old_sn = st.site_network
        n_sites = int(old_sn.n_sites)
        counts = st._device().site_counts(n_sites) if n_sites > 0 else np.zeros(0, dtype=np.int64)
        comm = st._comm
        if comm is not None and comm.size > 1:
            counts = comm.allreduce_sum(counts)
        seen_mask = counts > 0
        if np.all(seen_mask):
            return st
        logger.info("Removing unoccupied sites %s" % np.where(~seen_mask)[0])
        n_new_sites = int(np.sum(seen_mask))
        if n_new_sites < old_sn.n_mobile:                                    # :42-47
            raise errors.InsufficientSitesError(verb="Removing unoccupied sites", n_sites=n_new_sites,
                                                n_mobile=old_sn.n_mobile)
        translation = np.full(n_sites + 1, SiteTrajectory.SITE_UNKNOWN, dtype=np.int64)   # [-1]: unknown stays unknown
        translation[:-1][seen_mask] = np.arange(n_new_sites)
        new_st = st._derive(old_sn[seen_mask], translation[st._traj], None)
        if return_kept_sites:
            return new_st, np.where(seen_mask)
        return new_st


class _ReplaceWithCloser(object):
    """What ``ReplaceUnassignedPositions.replace_with_closer()`` returns: a replacement function that gives each frame of
    an unassigned run to whichever of the sites before and after the run the ion is closer to in real space."""

    def __init__(self):
        self._pbcc = None
        self._cell = None

    def __call__(self, st, mobile_atom, before_site, start_frame, after_site, end_frame):
        if before_site == SiteTrajectory.SITE_UNKNOWN or after_site == SiteTrajectory.SITE_UNKNOWN:
            return SiteTrajectory.SITE_UNKNOWN
        if st.real_trajectory is None:
            raise ValueError("replace_with_closer needs a SiteTrajectory with a real trajectory (set_real_traj)")
        sn = st.site_network
        cell = np.asarray(sn.structure.cell, dtype=np.float64)
        if self._pbcc is None or not np.array_equal(cell, self._cell):
            self._pbcc, self._cell = PBCCalculator(cell), cell.copy()
        atom = np.where(sn.mobile_mask)[0][mobile_atom]
        two = np.asarray(sn.centers)[[before_site, after_site]]
        out = np.empty(end_frame - start_frame, dtype=np.int64)
        for i in range(len(out)):
            d = self._pbcc.distances(st.real_trajectory[start_frame + i, atom], two)
            out[i] = before_site if d[0] < d[1] else after_site            # :83-86: a tie goes to the site after
        return out


def shard_halo(first_known, last_known, rank, none=-(1 << 63)):
    """``(before_in, after_in)`` of frame shard ``rank`` from the gathered ``label_ends()`` of all shards
    (``first_known`` / ``last_known``: ``[n_shards, n_mobile]``, ``none`` where a shard has no known label of the ion):
    per ion the last known label of the nearest lower shard that has one and the first known label of the nearest higher
    shard that has one, -1 where there is none."""
    first_known, last_known = np.asarray(first_known), np.asarray(last_known)
    M = first_known.shape[1]
    before = np.full(M, SiteTrajectory.SITE_UNKNOWN, dtype=np.int64)
    after = np.full(M, SiteTrajectory.SITE_UNKNOWN, dtype=np.int64)
    for r in range(rank):                                   # ascending: a nearer shard overwrites a further one
        has = last_known[r] != none
        before[has] = last_known[r][has]
    for r in range(len(first_known) - 1, rank, -1):
        has = first_known[r] != none
        after[has] = first_known[r][has]
    return before, after


class ReplaceUnassignedPositions(object):
    """Fills the runs of unassigned frames of every mobile ion from the sites on either side of the run (reference
    ``dynamics/ReplaceUnassignedPositions.py``).  ``run(st)`` returns a new ``SiteTrajectory``; ``st``, its label array
    and the labels resident on the device stay as they are.

    ``replacement_function``: a callable ``(st, mobile_atom, before_site, start_frame, after_site, end_frame)`` that
    returns one site for the whole run or an array of ``end_frame - start_frame`` sites.  ``before_site`` /
    ``after_site`` are the nearest labels other than ``SITE_UNKNOWN`` (-1 exactly) before and after the run,
    ``SITE_UNKNOWN`` where the trajectory begins or ends with the run.  The three strategies of the reference are
    recognised and evaluated by HIP kernels over the device-resident labels, without a pass of the host over the label
    array: ``replace_with_last_known``, ``replace_with_next_known`` (one call each) and the callable that
    ``replace_with_closer()`` makes (the runs come back as records, the positions of the frames to decide are gathered
    from ``st.real_trajectory`` with one fancy index, the decision is made on the device).  Any other callable is called
    once per run, ion by ion and in frame order, as the reference calls it.

    Deviations from the reference, whose own copy is barely usable:

    * ``None`` means ``replace_with_last_known``.  The reference's default reads an undefined ``RemoveShortJumps``
      (:42): ``ReplaceUnassignedPositions()`` raises ``NameError`` there.
    * ``replace_with_closer()`` returns a working callable.  The reference's returns ``None`` (:56-87: the inner
      function is never returned, and it assigns ``pbcc`` without ``nonlocal``).  The rule is that of its docstring and
      inner body: a frame goes to ``before_site`` when the ion is strictly closer to that centre (shift-and-wrap distance
      of ``PBCCalculator.distances``), otherwise to ``after_site``; a run with an unknown side stays unknown.  The ion's
      position is that of atom ``where(mobile_mask)[mobile_atom]`` of the real trajectory (the inner body indexes the
      real trajectory with the mobile-atom number itself, which is the ion only where the mobile atoms come first).  It
      raises ``ValueError`` without a real trajectory and ``IndexError`` for a label ``>= n_sites``; a label below -1
      is not wrapped round as numpy's indexing would, the device path refuses it with ``ValueError``.

    The result is ``st.copy(with_computed=False)`` of the reference with the new labels (:114-117): the confidences and
    the real trajectory are carried over; NO site or edge attribute is, computed or not - the reference's
    ``SiteNetwork.copy`` re-adds every attribute as "computed" (``SiteNetwork.py:116-123``) before it clears those, and
    the goldens record exactly that.

    On frame shards every rank calls ``label_ends()`` once, the ranks gather the two vectors and each derives what holds
    before its first and after its last frame (``shard_halo``); the three built-in strategies then run locally.  Another
    callable raises ``NotImplementedError`` there: a run would be cut at the ends of the shards."""

    def __init__(self, replacement_function=None):
        if replacement_function is None:
            replacement_function = ReplaceUnassignedPositions.replace_with_last_known
        assert callable(replacement_function)
        self.replacement_function = replacement_function

    @staticmethod
    def replace_with_last_known(st, mobile_atom, before_site, start_frame, after_site, end_frame):
        """Replace unassigned with the last known site."""
        return before_site

    @staticmethod
    def replace_with_next_known(st, mobile_atom, before_site, start_frame, after_site, end_frame):
        """Replace unassigned with the next known site."""
        return after_site

    @staticmethod
    def replace_with_closer():
        """Makes the function that assigns each position of an unassigned run to whichever of the sites before and after
        it is closer to in real space."""
        return _ReplaceWithCloser()

    def run(self, st):
        assert isinstance(st, SiteTrajectory)
        fn = self.replacement_function
        sn = st.site_network
        ctx = st._device()
        comm = st._comm
        before_in = after_in = None
        builtin = (fn is ReplaceUnassignedPositions.replace_with_last_known
                   or fn is ReplaceUnassignedPositions.replace_with_next_known or isinstance(fn, _ReplaceWithCloser))
        if comm is not None and comm.size > 1:
            if not builtin:
                raise NotImplementedError(
                    "ReplaceUnassignedPositions with a replacement function of the caller's is not available on frame "
                    "shards: a run of unassigned frames that crosses the end of a shard would be handed over in pieces")
            ends = comm.allgather(np.stack(ctx.label_ends()))               # [size, 2, n_mobile]
            before_in, after_in = shard_halo(ends[:, 0], ends[:, 1], comm.rank, ctx.ENDS_NONE)
        if fn is ReplaceUnassignedPositions.replace_with_last_known:
            out = ctx.replace_unassigned(0, before_in, after_in)
        elif fn is ReplaceUnassignedPositions.replace_with_next_known:
            out = ctx.replace_unassigned(1, before_in, after_in)
        elif isinstance(fn, _ReplaceWithCloser):
            if st.real_trajectory is None:
                raise ValueError("replace_with_closer needs a SiteTrajectory with a real trajectory (set_real_traj)")
            records, n_positions = ctx.unknown_runs(before_in, after_in)
            dec = records[records[:, 5] >= 0]
            lens = dec[:, 2] - dec[:, 1]
            # frame and atom of every position to decide, in record order: one gather, n_positions x 3
            within = np.arange(n_positions) - np.repeat(dec[:, 5], lens)
            frames = np.repeat(dec[:, 1] - ctx.frame0, lens) + within
            atoms = np.repeat(np.where(sn.mobile_mask)[0][dec[:, 0]], lens)
            positions = np.asarray(st.real_trajectory[frames, atoms], dtype=np.float64).reshape(-1, 3)
            centers = sn.centers if sn.n_sites > 0 else np.zeros((0, 3))
            out = ctx.replace_closer(records, centers, positions)
        else:
            records, _ = ctx.unknown_runs()
            out = st._traj.copy()
            for mob, start, end, before, after, _ in records:
                start, end = start - ctx.frame0, end - ctx.frame0          # frames of `st`, as the reference passes them
                out[start:end, mob] = fn(st, mob, before, start, after, end)        # :107-112
        # :114-117 (see the class docstring for what the reference's copy keeps)
        new_sn = sn.copy(with_computed=False)
        new_sn.clear_attributes()
        return st._derive(new_sn, out, st._confs)


def _selected_columns(traj, mask):
    """The front of a frame-series operator on a host trajectory: ``traj`` as an array, refused unless it is
    ``[n_frames, n_atoms, 3]`` float64, and ``traj[:, mask]``, contiguous - a copy: the caller's array stays as it is."""
    traj = np.asarray(traj)
    if traj.ndim != 3 or traj.shape[2] != 3:
        raise ValueError("Wrong shape %s for traj." % (traj.shape,))
    if traj.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % traj.dtype)
    selected = np.ascontiguousarray(traj[:, mask])
    if selected.ndim != 3:
        raise ValueError("`mask` must select along the atoms")
    return selected


def _resident_columns(la, mask, who):
    """The front on the frames an analysis left resident: ``(context, atom list)``; ``mask=None``: the mobile atoms."""
    la._need_run()
    if getattr(la, "_children", None) is not None or la._comm.size > 1 or la._ctx is None:
        raise NotImplementedError("%s needs all frames of the trajectory on one GPU; this analysis ran over frame shards" % who)
    if mask is None:
        return la._ctx, np.asarray(la._mobile_idx, dtype=np.int64)
    return la._ctx, np.arange(la._ctx.A, dtype=np.int64)[mask]      # numpy's rules: length, negative indices, bounds


class AverageVibrationalFrequency(object):
    """Average vibrational frequency of chosen atoms of a trajectory: the power spectrum of each atom's speed
    ``|x[t+1] - x[t]|`` gives a power-weighted mean frequency over ``min_frequency < f < max_frequency`` (units of
    1 / timestep; ``f = 0`` is always left out), and the result is the mean over the atoms (reference
    ``dynamics/AverageVibrationalFrequency.py``, after de Klerk, van der Maas and Wagemaker, ACS Appl. Energy Mater. 1
    (2018) 3230).  Its inverse is the mean vibrational period in frames: the threshold ``SmoothSiteTrajectory.run`` and
    ``assign_to_last_known_site`` are usually given.

    The speeds, the transform and the sums over the band are computed by HIP kernels (``sit_speed_spectrum``): the
    transform has the exact length ``n_frames - 1`` (Bluestein's algorithm in float64), every atom has its own, and the
    mean and standard deviation over the atoms are numpy's, on the host.

    Deviation from the reference: trajectories are float64 only.  The reference would compute the speeds of a float32
    trajectory in float32; here any other dtype raises the ``ValueError`` ``LandmarkAnalysis.run`` raises for its frames."""

    def __init__(self, min_frequency=0, max_frequency=np.inf):
        assert min_frequency >= 0                                  # the zero frequency is always excluded (:25-26)
        self.min_frequency = min_frequency
        self.max_frequency = max_frequency

    def _band(self, n_frames):
        if n_frames < 2:
            raise ValueError("A trajectory of %d frames has no speeds" % n_frames)
        freqs = np.fft.rfftfreq(n_frames - 1)                      # :43-45
        fmask = (freqs > self.min_frequency) & (freqs < self.max_frequency)
        assert np.any(fmask), "Trajectory too short?"
        return freqs, fmask

    @staticmethod
    def _over_atoms(avg_freqs, band_power, return_stdev):
        if np.any(band_power == 0.0):                              # np.average(freqs, weights = all zeros), :54
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        avg_freq = np.mean(avg_freqs)                              # :56-61
        if return_stdev:
            return avg_freq, np.std(avg_freqs)
        return avg_freq

    def compute_avg_vibrational_freq(self, traj, mask, return_stdev=False):
        """``traj``: a host trajectory ``[n_frames, n_atoms, 3]``, float64, not modified; ``mask``: the atoms to average
        over, a boolean mask or an index array (whatever ``traj[:, mask]`` takes).  Returns the frequency, with
        ``return_stdev`` ``(frequency, standard deviation over the atoms)``.

        Raises ``AssertionError("Trajectory too short?")`` when no frequency lies in the band (always with two frames),
        ``ValueError`` for fewer than two frames or another dtype, ``ZeroDivisionError`` when a chosen atom never
        moves (its band holds no power)."""
        selected = _selected_columns(traj, mask)
        freqs, fmask = self._band(len(selected))
        if selected.shape[1] == 0:
            return self._over_atoms(np.empty(0), np.empty(0), return_stdev)
        with _lib.HipContext(np.eye(3)) as ctx:                    # no cell enters: the differences are not wrapped
            avg_freqs, band_power, _, _ = ctx.speed_spectrum(freqs, fmask, positions=selected)
        return self._over_atoms(avg_freqs, band_power, return_stdev)

    def compute_for_analysis(self, la, mask=None, return_stdev=False):
        """The same from the trajectory a ``LandmarkAnalysis`` that has run left on its GPU: no upload, no gather on
        the host.  ``mask``: boolean mask or index array over the atoms of a frame; ``None``: the mobile atoms of the run.

        The frames are those ``run()`` received, as they were at that time: what the caller did to the array afterwards
        is not seen.  Raises ``ValueError`` if the analysis recentred the frames on the device (``recenter_masses``: a
        shift per frame changes the differences between frames, these are not the caller's frames any more) and
        ``NotImplementedError`` after a run over frame shards (``comm`` of more than one rank, ``devices=[...]`` of more
        than one GPU): a spectrum does not split over the frames."""
        ctx, atoms = _resident_columns(la, mask, "AverageVibrationalFrequency")
        if la._recenter_masses is not None:
            raise ValueError("The analysis recentred its frames on the device (recenter_masses): they are not the "
                             "trajectory run() was given; use compute_avg_vibrational_freq on that")
        freqs, fmask = self._band(ctx.F)
        if len(atoms) == 0:
            return self._over_atoms(np.empty(0), np.empty(0), return_stdev)
        avg_freqs, band_power, _, _ = ctx.speed_spectrum(freqs, fmask, atoms=atoms)
        return self._over_atoms(avg_freqs, band_power, return_stdev)


class GenerateClampedTrajectory(object):
    """A real-space trajectory in which the atoms of ``clamp_mask`` stand on fixed positions: a static atom on its
    position in the network's structure, a mobile atom on the centre of the site it is assigned to at that frame; every
    other atom keeps its real position (reference ``misc/GenerateClampedTrajectory.pyx``).

    ``wrap``: ``True`` writes the centres as they are; ``False`` (the default) the periodic image of the centre nearest
    the atom's real position, which turns an unwrapped real trajectory into an unwrapped clamped one.
    ``pass_through_unassigned``: ``True`` writes the real position of a mobile atom to clamp at the frames where it is
    unassigned; ``False`` raises the reference's ``RuntimeError`` when there is such a frame.

    One HIP kernel (``sit_clamp_trajectory``) makes every frame from the device-resident labels, in chunks of frames that
    are copied back as they are finished; the arithmetic of a clamped point follows the reference operation by operation
    and the result is bit-equal to it wherever the reference runs.

    Deviations from the reference, whose own copy does not get far:

    * The stock module is rejected by Cython 3 (``:117``), and once compiled ``run()`` raises ``IndexError`` at ``:71``
      for every structure with a static atom: it indexes the ``n_mobile`` label columns with a mask over all atoms, and
      its loop (``:94-99``) reads the label column with the atom's index.  Here the label column of a mobile atom is its
      rank among the mobile atoms, which is what the docstring describes and what the reference does where it runs
      (every atom mobile).
    * A mask that selects no mobile atom is valid.  The reference raises numpy's ``ValueError`` for the minimum of an
      empty array (``:73``).
    * A clamped atom that is neither static nor mobile gets its position in the structure; the reference leaves its
      entries of ``np.empty`` as they are.
    * Without a real trajectory, a mobile atom to clamp that needs its real position (``wrap=False``, or an unassigned
      frame to pass through) raises ``RuntimeError``; the reference dereferences ``None``.
    * Trajectories are float64 only: another dtype raises the ``ValueError`` ``AverageVibrationalFrequency`` raises.
    * A label ``>= n_sites`` raises ``IndexError`` (the reference reads past the centre table), a label below -1
      ``ValueError``.
    * On frame shards ``run(st)`` clamps the frames of its shard; nothing is exchanged and nothing gathered."""

    NO_REAL_TRAJ_MSG = ("This `SiteTrajectory` has no real-space trajectory, but the given clamp mask leaves some atoms "
                        "unclamped.")

    def __init__(self, wrap=False, pass_through_unassigned=False):
        self.wrap = wrap
        self.pass_through_unassigned = pass_through_unassigned

    @staticmethod
    def _roles(sn, clamp_mask):
        """``(role[n_atoms] int32, clamp_mask)``: -1 pass through, -2 the structure's position, ``m >= 0`` label column
        ``m`` - the rank of the atom among the mobile ones."""
        n_atoms = len(sn.structure)
        if clamp_mask is None:
            clamp_mask = np.ones(n_atoms, dtype=bool)
        clamp_mask = np.asarray(clamp_mask)
        if clamp_mask.dtype != np.bool_ or clamp_mask.shape != (n_atoms,):
            raise ValueError("clamp_mask must be a boolean mask over the %d atoms of the structure" % n_atoms)
        mobile = np.asarray(sn.mobile_mask, dtype=bool)
        role = np.full(n_atoms, -1, dtype=np.int32)
        role[clamp_mask] = -2
        rank = np.cumsum(mobile) - 1
        sel = clamp_mask & mobile
        role[sel] = rank[sel]
        return role, clamp_mask

    def _call(self, ctx, sn, role, positions, have_positions):
        centers = np.asarray(sn.centers, dtype=np.float64).reshape(-1, 3) if sn.n_sites > 0 else np.zeros((0, 3))
        fixed = np.asarray(sn.structure.get_positions(), dtype=np.float64)
        clamps_mobile = bool(np.any(role >= 0))
        if not have_positions:
            if np.any(role == -1):
                raise RuntimeError(self.NO_REAL_TRAJ_MSG)                                # :59-60
            if clamps_mobile and not self.wrap:
                raise RuntimeError("This `SiteTrajectory` has no real-space trajectory, which clamping with wrap=False "
                                   "needs for every mobile atom to clamp.")
            try:
                # nothing to read but labels and centres; an unassigned label shows in the same pass
                return ctx.clamp_trajectory(role, fixed, centers, True, False)
            except errors.UnassignedClampError:
                if not self.pass_through_unassigned:
                    raise
                raise RuntimeError("This `SiteTrajectory` has no real-space trajectory, but a mobile atom to clamp is "
                                   "unassigned at some frame and `pass_through_unassigned` would pass its position through.")
        return ctx.clamp_trajectory(role, fixed, centers, self.wrap, self.pass_through_unassigned, positions=positions)

    def run(self, st, clamp_mask=None):
        """``float64[n_frames, n_atoms, 3]``.  ``clamp_mask``: boolean over the atoms of the structure, any mixture of
        static and mobile ones; ``None``: all.  The labels are the trajectory's (``st._device()``), the positions
        ``st.real_trajectory``; nothing of it is sent to the GPU when no element needs a real position (``wrap=True``,
        every atom clamped, no pass-through)."""
        assert isinstance(st, SiteTrajectory)
        sn = st.site_network
        role, clamp_mask = self._roles(sn, clamp_mask)
        real = st.real_trajectory
        if real is None and not np.all(clamp_mask):
            raise RuntimeError(self.NO_REAL_TRAJ_MSG)
        if real is not None:
            real = np.asarray(real)
            if real.dtype != np.float64:
                raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % real.dtype)
        ctx = st._device()
        needs = bool(np.any(role == -1)) or (bool(np.any(role >= 0)) and (not self.wrap or self.pass_through_unassigned))
        if real is not None and not needs:
            return ctx.clamp_trajectory(role, np.asarray(sn.structure.get_positions(), dtype=np.float64),
                                        np.asarray(sn.centers, dtype=np.float64).reshape(-1, 3) if sn.n_sites > 0
                                        else np.zeros((0, 3)), True, False)
        return self._call(ctx, sn, role, real, real is not None)

    def run_for_analysis(self, la, st=None, clamp_mask=None):
        """The same from the frames a ``LandmarkAnalysis`` that has run left on its GPU: no upload.  ``st``: the
        trajectory to take the labels from - ``None``: the one ``la.run()`` returned; otherwise one that shares the
        analysis' device context (that trajectory after ``assign_to_last_known_site`` or an edit of ``st.traj``, a copy
        ``st[:]``), whose labels are brought up to date on the device first.  A trajectory with a context of its own (the
        result of ``SmoothSiteTrajectory`` or ``ReplaceUnassignedPositions``, one made by the caller) raises
        ``ValueError``: use ``run(st)`` with its real trajectory.

        The frames are those ``run()`` received, as they were at that time.  Raises ``ValueError`` if the analysis
        recentred the frames on the device (``recenter_masses``) and ``NotImplementedError`` after a run over frame shards
        (``comm`` of more than one rank, ``devices=[...]``), as ``AverageVibrationalFrequency.compute_for_analysis``."""
        la._need_run()
        if getattr(la, "_children", None) is not None or la._comm.size > 1 or la._ctx is None:
            raise NotImplementedError("GenerateClampedTrajectory.run_for_analysis needs all frames of the trajectory on "
                                      "one GPU; this analysis ran over frame shards (use run(st) on every shard)")
        if la._recenter_masses is not None:
            raise ValueError("The analysis recentred its frames on the device (recenter_masses): they are not the "
                             "trajectory run() was given; use run(st) on that")
        if st is None:
            ref = getattr(la, "_result", None)
            st = ref() if ref is not None else None
            if st is None:
                raise ValueError("The trajectory this analysis returned does not exist any more; pass `st`")
        assert isinstance(st, SiteTrajectory)
        if st._ctx is not la._ctx:
            raise ValueError("`st` does not share the device context of this analysis; use run(st)")
        sn = st.site_network
        role, _ = self._roles(sn, clamp_mask)
        ctx = st._device()
        if len(role) != ctx.A:
            raise ValueError("The structure has %d atoms, the resident frames %d" % (len(role), ctx.A))
        return self._call(ctx, sn, role, None, True)


class MSDResult(object):
    """What ``MeanSquaredDisplacement`` returns.

    ``lags`` int64 ``[n_lags]`` (frames); ``msd_axes`` ``[n_sel, n_lags, 3]`` per atom and Cartesian axis; ``msd``
    ``[n_sel, n_lags]`` their sum over the axes; ``mean`` ``[n_lags]`` its mean over the atoms (the tracer MSD);
    ``collective`` ``[n_lags, 3]`` (the MSD of the summed displacement divided by the number of atoms: its ratio to the
    tracer MSD is the Haven ratio) or ``None``; ``alpha2`` ``[n_sel, n_lags]`` the non-Gaussian parameter
    ``3 <r^4> / (5 <r^2>^2) - 1`` (explicit lags only, else ``None``; NaN at lag 0); ``max_residual`` the largest distance
    of a step from a whole number of cell vectors, in units of them; ``images`` int32 ``[n_sel, n_frames, 3]`` the image
    counts of the unwrapping (only when asked for, else ``None``)."""

    def __init__(self, lags, msd_axes, collective, r4, max_residual, images):
        self.lags = lags
        self.msd_axes = msd_axes
        self.msd = (msd_axes[..., 0] + msd_axes[..., 1]) + msd_axes[..., 2]
        self.mean = np.mean(self.msd, axis=0) if len(self.msd) else np.full(len(lags), np.nan)
        self.collective = collective
        self.r4 = r4
        if r4 is None:
            self.alpha2 = None
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                self.alpha2 = 3.0 * r4 / (5.0 * self.msd * self.msd) - 1.0
        self.max_residual = max_residual
        self.images = images


def diffusion_coefficient(lags, msd, timestep=1.0, fit_range=None, dimensions=3):
    """``(D, intercept)``: ordinary least squares of ``msd`` on ``lags * timestep`` with an intercept,
    ``D = slope / (2 * dimensions)`` (Einstein's relation).  ``fit_range``: ``(first, last)`` lag, inclusive, in frames;
    ``None``: every lag given.  Host numpy."""
    lags = np.asarray(lags, dtype=np.float64)
    msd = np.asarray(msd, dtype=np.float64)
    if lags.shape != msd.shape or lags.ndim != 1:
        raise ValueError("lags and msd must be one-dimensional and of one length")
    if fit_range is not None:
        keep = (lags >= fit_range[0]) & (lags <= fit_range[1])
        lags, msd = lags[keep], msd[keep]
    if len(lags) < 2:
        raise ValueError("A fit needs at least two lags")
    t = lags * timestep
    tm, mm = np.mean(t), np.mean(msd)
    slope = np.sum((t - tm) * (msd - mm)) / np.sum((t - tm) * (t - tm))
    return slope / (2 * dimensions), mm - slope * tm


class MeanSquaredDisplacement(object):
    """Mean squared displacement of chosen atoms against the lag time, per atom and Cartesian axis: the tracer MSD, from
    which ``diffusion_coefficient`` fits D, and with ``collective`` the MSD of the summed displacement (the "charge" MSD;
    its ratio to the tracer one is the Haven ratio).  The reference has no such operator; the definitions are in
    ``DESIGN.md`` section 20.

    ``max_lag``: all lags ``0 .. max_lag`` (``None``: ``n_frames // 2``), by the autocorrelation of every unwrapped series
    through a zero-padded float64 transform and a windowed sum (``sit_msd``: O(F log F) per atom and axis).  ``lags``:
    instead, the lags listed (log-spaced ones, say), by the sums themselves, one workgroup per (lag, atom); this path also
    gives the non-Gaussian parameter ``alpha2``.  ``unwrap``: the trajectory is unwrapped under the cell first - a step is
    taken to cross the whole number of cell vectors nearest to it, which is right for any cell shape while no atom moves
    half a cell vector or more between two frames; ``MSDResult.max_residual`` says how close the trajectory came, and a
    value above 0.25 logs a warning.  A trajectory that is unwrapped already passes through bit for bit.

    The site-hop MSD (displacements counted from site centre to site centre) is this operator applied to the output of
    ``GenerateClampedTrajectory(wrap=False)``."""

    def __init__(self, max_lag=None, lags=None, unwrap=True, collective=False):
        if max_lag is not None and lags is not None:
            raise ValueError("Give max_lag or lags, not both")
        self.max_lag = max_lag
        self.lags = None if lags is None else np.array(lags, dtype=np.int64).reshape(-1)
        self.unwrap = unwrap
        self.collective = collective

    def _result(self, n_frames, raw):
        msd, r4, coll, images, max_residual = raw
        lags = self.lags if self.lags is not None else np.arange(msd.shape[2], dtype=np.int64)
        if max_residual > 0.25:
            logger.warning("MeanSquaredDisplacement: a step of %.3f cell vectors from the nearest whole number of them - a "
                           "step of a quarter of the cell is not molecular dynamics; the unwrapping may be wrong."
                           % max_residual)
        return MSDResult(lags, np.ascontiguousarray(msd.transpose(0, 2, 1)), None if coll is None else np.ascontiguousarray(coll.T),
                         r4, max_residual, images)

    def _empty(self, n_frames, images):
        if n_frames < 2:
            raise ValueError("A trajectory of %d frames has no displacements" % n_frames)
        n_lags = len(self.lags) if self.lags is not None else (n_frames // 2 if self.max_lag is None else self.max_lag) + 1
        raw = (np.zeros((0, 3, n_lags)), np.zeros((0, n_lags)) if self.lags is not None else None,
               np.full((3, n_lags), np.nan) if self.collective else None,
               np.zeros((0, n_frames, 3), dtype=np.int32) if images else None, 0.0)
        return self._result(n_frames, raw)

    def _call(self, ctx, images, **kw):
        return ctx.msd(unwrap=self.unwrap, max_lag=self.max_lag, lags=self.lags, collective=self.collective,
                       r4=self.lags is not None, images=images, **kw)

    def compute(self, traj, cell, mask, images=False):
        """``traj``: a host trajectory ``[n_frames, n_atoms, 3]``, float64, not modified; ``cell``: rows are the cell
        vectors (looked at only with ``unwrap``); ``mask``: the atoms, a boolean mask or an index array (whatever
        ``traj[:, mask]`` takes).  Returns an ``MSDResult``.  ``ValueError`` for fewer than two frames, another dtype, a lag
        beyond ``n_frames - 1`` or a degenerate cell."""
        selected = _selected_columns(traj, mask)
        if selected.shape[1] == 0:
            return self._empty(len(selected), images)
        with _lib.HipContext(np.asarray(cell, dtype=np.float64) if self.unwrap else np.eye(3)) as ctx:
            raw = self._call(ctx, images, positions=selected)
        return self._result(len(selected), raw)

    def compute_for_analysis(self, la, mask=None, images=False):
        """The same from the trajectory a ``LandmarkAnalysis`` that has run left on its GPU, under that analysis' cell: no
        upload, no gather on the host.  ``mask``: boolean mask or index array over the atoms of a frame; ``None``: the
        mobile atoms of the run.

        The frames are those ``run()`` received, as they were at that time.  Frames the analysis recentred on the device
        (``recenter_masses``) are accepted: they are the trajectory relative to the framework's centre of mass, and an MSD
        relative to the framework is what one wants from a cell that drifts.  ``NotImplementedError`` after a run over
        frame shards (``comm`` of more than one rank, ``devices=[...]`` of more than one GPU): a lag reaches across the
        shards."""
        ctx, atoms = _resident_columns(la, mask, "MeanSquaredDisplacement")
        if len(atoms) == 0:
            return self._empty(ctx.F, images)
        return self._result(ctx.F, self._call(ctx, images, atoms=atoms))


class VanHoveResult(object):
    """What ``VanHoveCorrelation`` returns.

    ``lags`` int64 ``[n_lags]`` (frames); ``edges`` ``[n_bins + 1]`` and ``r`` ``[n_bins]``, the bin edges and centres;
    ``n_origins`` int64 ``[n_lags]``, the time origins of every lag; ``self_counts`` / ``distinct_counts`` uint64
    ``[n_lags, n_bins + 1]`` as the device counted them, the last entry of a row being the overflow (everything at ``r_max``
    or beyond, or not finite); ``self_density`` ``[n_lags, n_bins]`` = counts / (origins * n_a * dr), the probability density of
    the displacement length ``4 pi r^2 G_s(r, tau)``, which integrates to one minus the overflow share; ``distinct``
    ``[n_lags, n_bins]`` = counts * V / (origins * pairs * volume of the shell) = ``G_d(r, tau) / rho``, which is ``g(r)`` at lag
    0.  A part that was not asked for is ``None``.  ``max_residual``: as ``MSDResult.max_residual`` (0 without unwrapping)."""

    def __init__(self, lags, edges, n_origins, n_a, n_pairs, volume, self_counts, distinct_counts, max_residual):
        self.lags, self.edges, self.n_origins = lags, edges, n_origins
        self.r = 0.5 * (edges[:-1] + edges[1:])
        self.self_counts, self.distinct_counts, self.max_residual = self_counts, distinct_counts, max_residual
        self.n_a, self.n_pairs = n_a, n_pairs
        n_bins = len(edges) - 1
        dr = edges[-1] / n_bins
        shells = (4.0 * np.pi / 3.0) * (edges[1:] ** 3 - edges[:-1] ** 3)
        origins = n_origins.astype(np.float64)[:, None]
        self.self_density = self.distinct = None
        with np.errstate(divide="ignore", invalid="ignore"):
            if self_counts is not None:
                self.self_density = self_counts[:, :n_bins] / (origins * n_a * dr)
            if distinct_counts is not None:
                self.distinct = distinct_counts[:, :n_bins] * volume / (origins * n_pairs * shells[None, :])


def _vanhove_edges(r_max, n_bins):
    edges = np.arange(n_bins + 1, dtype=np.float64) * (float(r_max) / n_bins)
    edges[-1] = float(r_max)
    return edges


class VanHoveCorrelation(object):
    """The van Hove correlation function of chosen atoms against the lag time, as histograms of distances: the self part
    ``G_s(r, tau)``, the distribution of ``|x_i(t + tau) - x_i(t)|`` (its peaks at the site-to-site distances show hopping), and
    the distinct part ``G_d(r, tau)``, the distribution of ``|x_j(t + tau) - x_i(t)|`` over the pairs ``i != j`` of two
    selections (at small ``r``: does an ion move into the place another one left).  The reference has no such operator; the
    definitions are in ``DESIGN.md`` section 21.

    ``lags``: the lags, in frames, each in ``[0, n_frames - 1]``.  ``r_max``, ``n_bins``: bins of equal width on
    ``[0, r_max)``; ``r_max`` is at most half the smallest perpendicular height of the cell (less one part in 2^30), where
    the rounded fractional difference is the true minimum image for any cell shape.  ``origin_stride``: every how many frames
    a time origin is taken.  ``unwrap``: the self part follows the trajectory unwrapped under the cell as
    ``MeanSquaredDisplacement`` does (``max_residual`` above 0.25 logs its warning); the distinct part reads the frames as
    they are.  The counts come from HIP kernels (``sit_vanhove``) as integers added with integer atomics - the same bytes on
    every call - and are normalised on the host in float64."""

    def __init__(self, lags, r_max, n_bins, origin_stride=1, self_part=True, distinct_part=True, unwrap=True):
        self.lags = np.array(lags, dtype=np.int64).reshape(-1)
        self.r_max, self.n_bins, self.origin_stride = float(r_max), int(n_bins), int(origin_stride)
        self.self_part, self.distinct_part, self.unwrap = bool(self_part), bool(distinct_part), bool(unwrap)
        if not (self.self_part or self.distinct_part):
            raise ValueError("Neither the self part nor the distinct part is asked for")
        if self.n_bins < 1 or self.origin_stride < 1 or len(self.lags) < 1:
            raise ValueError("n_bins, origin_stride and the number of lags must be at least 1")

    def _run(self, ctx, a, b, same, n_frames, positions=None):
        from . import _lib_vanhove
        if len(a) == 0 or len(b) == 0:
            raise ValueError("A selection holds no atom")
        sc, dc, res = _lib_vanhove.vanhove(ctx, a, b, self.lags, self.r_max, self.n_bins, positions=positions, same=same,
                                           origin_stride=self.origin_stride, unwrap=self.unwrap, self_part=self.self_part,
                                           distinct_part=self.distinct_part)
        if self.unwrap and self.self_part and res > 0.25:
            logger.warning("VanHoveCorrelation: a step of %.3f cell vectors from the nearest whole number of them - a "
                           "step of a quarter of the cell is not molecular dynamics; the unwrapping may be wrong." % res)
        n_origins = (n_frames - 1 - self.lags) // self.origin_stride + 1
        n_pairs = len(a) * len(b) - (len(a) if same else 0)
        return VanHoveResult(self.lags, _vanhove_edges(self.r_max, self.n_bins), n_origins, len(a), n_pairs,
                             abs(float(np.linalg.det(ctx.cell))), sc, dc, res)

    def compute(self, traj, cell, mask, mask_b=None):
        """``traj``: a host trajectory ``[n_frames, n_atoms, 3]``, float64, not modified; ``cell``: rows are the cell vectors;
        ``mask`` / ``mask_b``: the two selections, boolean masks or index arrays (whatever ``traj[:, mask]`` takes);
        ``mask_b=None``: the same selection, pairs of an atom with itself left out.  Returns a ``VanHoveResult``.
        ``ValueError`` for another dtype, an empty selection, a lag beyond ``n_frames - 1``, ``r_max`` beyond half the
        smallest height of the cell or a degenerate cell."""
        sel = _selected_columns(traj, mask)
        n_a = sel.shape[1]
        a = b = np.arange(n_a, dtype=np.int64)
        if mask_b is not None:
            sel_b = _selected_columns(traj, mask_b)
            b = n_a + np.arange(sel_b.shape[1], dtype=np.int64)
            sel = np.ascontiguousarray(np.concatenate([sel, sel_b], axis=1))
        with _lib.HipContext(np.asarray(cell, dtype=np.float64)) as ctx:
            return self._run(ctx, a, b, mask_b is None, len(sel), positions=sel)

    def compute_for_analysis(self, la, mask=None, mask_b=None):
        """The same from the trajectory a ``LandmarkAnalysis`` that has run left on its GPU, under that analysis' cell: no
        upload.  ``mask``: boolean mask or index array over the atoms of a frame, ``None``: the mobile atoms of the run;
        ``mask_b=None``: the same selection.  Frames the analysis recentred on the device are accepted, as
        ``MeanSquaredDisplacement.compute_for_analysis`` accepts them; ``NotImplementedError`` after a run over frame shards."""
        ctx, a = _resident_columns(la, mask, "VanHoveCorrelation")
        b = a if mask_b is None else _resident_columns(la, mask_b, "VanHoveCorrelation")[1]
        return self._run(ctx, a, b, mask_b is None, ctx.F)


class RDFResult(object):
    """What ``RadialDistribution`` returns: ``r`` ``[n_bins]`` and ``edges`` ``[n_bins + 1]``; ``g`` ``[n_bins]``, the radial
    distribution function of the ``b`` atoms around the ``a`` atoms; ``counts`` uint64 ``[n_bins + 1]`` as the device counted
    them over all frames taken (the last entry: pairs at ``r_max`` or beyond); ``n`` ``[n_bins]``, the running coordination
    number ``cumsum(counts) / (frames taken * n_a)`` at the upper edge of every bin; ``n_origins``, the frames taken."""

    def __init__(self, vh):
        self.r, self.edges = vh.r, vh.edges
        self.g, self.counts, self.n_origins = vh.distinct[0], vh.distinct_counts[0], int(vh.n_origins[0])
        self.n = np.cumsum(self.counts[:-1]) / (float(self.n_origins) * vh.n_a)


class RadialDistribution(object):
    """The radial distribution function ``g(r)`` between two selections of atoms, averaged over every ``frame_stride``-th
    frame: the distinct part of ``VanHoveCorrelation`` at lag 0 alone, by the same kernels; ``r_max`` and ``n_bins`` as there."""

    def __init__(self, r_max, n_bins, frame_stride=1):
        self._vh = VanHoveCorrelation([0], r_max, n_bins, origin_stride=frame_stride, self_part=False, unwrap=False)

    def compute(self, traj, cell, mask_a, mask_b=None):
        """``mask_b=None``: among the atoms of ``mask_a``.  Returns an ``RDFResult``; the errors of ``VanHoveCorrelation.compute``."""
        return RDFResult(self._vh.compute(traj, cell, mask_a, mask_b))

    def compute_for_analysis(self, la, mask_a=None, mask_b="static"):
        """From the frames an analysis left resident.  ``mask_a=None``: the mobile atoms; ``mask_b``: ``"static"`` for the static
        atoms of the run, ``None`` for the atoms of ``mask_a``, else a mask or an index array."""
        if isinstance(mask_b, str):
            if mask_b != "static":
                raise ValueError("mask_b is a mask, an index array, None or \"static\"")
            _resident_columns(la, mask_a, "RadialDistribution")      # has run, on one GPU
            mask_b = np.asarray(la._static_idx, dtype=np.int64)
        return RDFResult(self._vh.compute_for_analysis(la, mask_a, mask_b))


def q_vectors(cell, q_max, half_space=True):
    """The integer triples ``(h, k, l)`` int64 ``[n_q, 3]`` of the q vectors ``q = 2 pi (h ci[0] + k ci[1] + l ci[2])``
    (``ci = inverse(cell^T)``: the reciprocal lattice of the cell, the only q vectors a periodic trajectory defines without
    unwrapping) with ``0 < |q| <= q_max``, ordered by ``|q|`` and then by index.  ``half_space``: one of every pair ``+-q`` - the
    one whose first non-zero index is positive - since ``F(-q, tau) = conj F(q, tau)``.  ``ValueError`` for a ``q_max`` that needs
    an index beyond 32, with the number of cell lengths it asks for."""
    cell = np.asarray(cell, dtype=np.float64)
    q_max = float(q_max)
    if cell.shape != (3, 3) or not q_max > 0.0 or not np.isfinite(q_max):
        raise ValueError("q_vectors needs a 3 x 3 cell and a finite q_max above 0")
    recip = 2.0 * np.pi * np.linalg.inv(cell.T)                       # rows: 2 pi ci[a]
    # |index a| <= q_max |c_a| / (2 pi): q . c_a = 2 pi (index a) and |q . c_a| <= |q| |c_a|
    need = np.floor(q_max * np.linalg.norm(cell, axis=1) / (2.0 * np.pi) * (1.0 + 1e-12)).astype(np.int64)
    if np.any(need > 32):
        raise ValueError("q_max = %g needs an index of %d along a cell vector: a wavelength of 1/%d of that cell length, beyond "
                         "the 32 the device tables hold" % (q_max, need.max(), need.max()))
    grids = np.meshgrid(*[np.arange(-n, n + 1) for n in need], indexing="ij")
    hkl = np.stack([g.reshape(-1) for g in grids], axis=1).astype(np.int64)
    norm = np.linalg.norm(hkl.astype(np.float64) @ recip, axis=1)
    keep = (norm <= q_max) & np.any(hkl != 0, axis=1)
    if half_space:
        first = hkl[np.arange(len(hkl)), np.argmax(hkl != 0, axis=1)]
        keep &= first > 0
    hkl, norm = hkl[keep], norm[keep]
    order = np.lexsort((hkl[:, 2], hkl[:, 1], hkl[:, 0], norm))
    return np.ascontiguousarray(hkl[order])


def _shell_average(q_norm, values, edges):
    """``(mean [..., n_bins], count [n_bins])`` of ``values [..., n_q]`` over the q vectors of every bin ``edges[k] <= |q| <
    edges[k + 1]``; NaN where a bin holds none."""
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    which = np.searchsorted(edges, q_norm, "right") - 1
    n_bins = len(edges) - 1
    inside = (which >= 0) & (which < n_bins)
    count = np.bincount(which[inside], minlength=n_bins)
    values = np.asarray(values)
    out = np.full(values.shape[:-1] + (n_bins,), np.nan, dtype=values.dtype)
    for k in np.nonzero(count)[0]:
        out[..., k] = values[..., inside & (which == k)].mean(axis=-1)
    return out, count


class ScatteringResult(object):
    """What ``IntermediateScattering`` returns.

    ``q_int`` int64 ``[n_q, 3]``, ``q`` ``[n_q, 3]`` the Cartesian vectors and ``q_norm`` ``[n_q]``; ``lags`` int64 ``[n_lags]``
    and ``n_origins`` int64 ``[n_lags]``; ``self_sums`` / ``coherent_sums`` complex128 ``[n_lags, n_q]`` as the device summed
    them; ``self`` = sums / (origins n_a), ``coherent`` = sums / (origins sqrt(n_a n_b)) and, for one selection, ``distinct`` =
    coherent - self.  A part that was not asked for, or is not defined, is ``None``."""

    def __init__(self, q_int, cell, lags, n_origins, n_a, n_b, same, self_sums, coherent_sums):
        self.q_int, self.lags, self.n_origins = q_int, lags, n_origins
        self.q = q_int.astype(np.float64) @ (2.0 * np.pi * np.linalg.inv(np.asarray(cell, dtype=np.float64).T))
        self.q_norm = np.linalg.norm(self.q, axis=1)
        self.n_a, self.n_b = n_a, n_b
        self.self_sums, self.coherent_sums = self_sums, coherent_sums
        origins = n_origins.astype(np.float64)[:, None]
        self.self = None if self_sums is None else self_sums / (origins * n_a)
        self.coherent = None if coherent_sums is None else coherent_sums / (origins * np.sqrt(float(n_a) * float(n_b)))
        self.distinct = self.coherent - self.self if (same and self.self is not None and self.coherent is not None) else None

    def shell_average(self, edges):
        """``(self, coherent, distinct, count)``: the mean of each part ``[n_lags, n_bins]`` over the q vectors whose ``|q|`` lies
        in every bin of ``edges`` (``None`` for a part that is), and the q vectors per bin; NaN where a bin holds none."""
        parts = [None if v is None else _shell_average(self.q_norm, v, edges)[0] for v in (self.self, self.coherent, self.distinct)]
        return parts[0], parts[1], parts[2], _shell_average(self.q_norm, np.zeros(len(self.q_norm)), edges)[1]


class IntermediateScattering(object):
    """The intermediate scattering function of chosen atoms over q vectors commensurate with the cell: the self part
    ``F_s(q, tau)`` = mean over atoms and origins of ``exp(i q . (x_i(t + tau) - x_i(t)))`` (what quasi-elastic neutron scattering
    measures; its decay against ``|q|`` confronts a hopping model with the trajectory) and the coherent part ``F(q, tau)`` =
    ``<rho_b(q, t + tau) conj rho_a(q, t)> / sqrt(n_a n_b)`` with ``rho(q, t) = sum_i exp(i q . x_i(t))``, whose lag-0 value is
    the static structure factor.  The reference has no such operator; the definitions are in ``DESIGN.md`` section 22.

    ``q_int``: integer triples ``[n_q, 3]``, each index within +-32 (``q_vectors`` makes them); ``lags``: the lags, in frames,
    each in ``[0, n_frames - 1]``; ``origin_stride``: every how many frames a time origin is taken.  For these q vectors the
    phase of an atom does not change when it moves by a cell vector, so the trajectory is read as it is, wrapped or not.  The
    sums come from HIP kernels (``sit_scattering``) in float64 with a sine and cosine of the library's own and a fixed order - the
    same bytes on every call - and are normalised on the host."""

    def __init__(self, q_int, lags, origin_stride=1, self_part=True, coherent_part=True):
        self.q_int = np.ascontiguousarray(np.array(q_int, dtype=np.int64).reshape(-1, 3))
        self.lags = np.array(lags, dtype=np.int64).reshape(-1)
        self.origin_stride = int(origin_stride)
        self.self_part, self.coherent_part = bool(self_part), bool(coherent_part)
        if not (self.self_part or self.coherent_part):
            raise ValueError("Neither the self part nor the coherent part is asked for")
        if len(self.q_int) < 1 or self.origin_stride < 1 or len(self.lags) < 1:
            raise ValueError("The number of q vectors, origin_stride and the number of lags must be at least 1")

    def _run(self, ctx, a, b, same, n_frames, positions=None):
        from . import _lib_scattering
        if len(a) == 0 or len(b) == 0:
            raise ValueError("A selection holds no atom")
        if self.self_part and not same:
            raise ValueError("The self part is that of one selection: leave mask_b out, or ask for self_part=False")
        ss, cs = _lib_scattering.scattering(ctx, a, b, self.q_int, self.lags, positions=positions, same=same,
                                            origin_stride=self.origin_stride, self_part=self.self_part, coherent_part=self.coherent_part)
        n_origins = (n_frames - 1 - self.lags) // self.origin_stride + 1
        return ScatteringResult(self.q_int, ctx.cell, self.lags, n_origins, len(a), len(b), same, ss, cs)

    def compute(self, traj, cell, mask, mask_b=None):
        """``traj``: a host trajectory ``[n_frames, n_atoms, 3]``, float64, not modified; ``cell``: rows are the cell vectors;
        ``mask`` / ``mask_b``: the selections, boolean masks or index arrays (whatever ``traj[:, mask]`` takes); ``mask_b=None``:
        one selection.  Returns a ``ScatteringResult``.  ``ValueError`` for another dtype, an empty selection, a lag beyond
        ``n_frames - 1``, an index beyond 32, a degenerate cell, or the self part with ``mask_b`` given."""
        sel = _selected_columns(traj, mask)
        n_a = sel.shape[1]
        a = b = np.arange(n_a, dtype=np.int64)
        if mask_b is not None:
            sel_b = _selected_columns(traj, mask_b)
            b = n_a + np.arange(sel_b.shape[1], dtype=np.int64)
            sel = np.ascontiguousarray(np.concatenate([sel, sel_b], axis=1))
        with _lib.HipContext(np.asarray(cell, dtype=np.float64)) as ctx:
            return self._run(ctx, a, b, mask_b is None, len(sel), positions=sel)

    def compute_for_analysis(self, la, mask=None, mask_b=None):
        """The same from the trajectory a ``LandmarkAnalysis`` that has run left on its GPU, under that analysis' cell: no
        upload.  ``mask``: boolean mask or index array over the atoms of a frame, ``None``: the mobile atoms of the run;
        ``mask_b=None``: the same selection.  ``NotImplementedError`` after a run over frame shards."""
        ctx, a = _resident_columns(la, mask, "IntermediateScattering")
        b = a if mask_b is None else _resident_columns(la, mask_b, "IntermediateScattering")[1]
        return self._run(ctx, a, b, mask_b is None, ctx.F)


class StructureFactorResult(object):
    """What ``StructureFactor`` returns: ``q_int``, ``q``, ``q_norm`` as ``ScatteringResult``; ``S`` ``[n_q]``, real for one
    selection (``<|rho(q)|^2> / n``) and complex for a partial between two; ``sums`` complex128 ``[n_q]`` as the device summed
    them; ``n_origins``, the frames taken; ``shell_average(edges)`` -> ``(mean of S per |q| bin, q vectors per bin)``."""

    def __init__(self, res, same):
        self.q_int, self.q, self.q_norm = res.q_int, res.q, res.q_norm
        self.sums, self.n_origins = res.coherent_sums[0], int(res.n_origins[0])
        self.S = res.coherent[0].real.copy() if same else res.coherent[0]

    def shell_average(self, edges):
        return _shell_average(self.q_norm, self.S, edges)


class StructureFactor(object):
    """The static structure factor ``S(q)`` of a selection, or the partial one between two, averaged over every
    ``frame_stride``-th frame: the coherent part of ``IntermediateScattering`` at lag 0 alone, by the same kernels."""

    def __init__(self, q_int, frame_stride=1):
        self._isf = IntermediateScattering(q_int, [0], origin_stride=frame_stride, self_part=False)

    def compute(self, traj, cell, mask_a, mask_b=None):
        """``mask_b=None``: the atoms of ``mask_a`` among themselves.  The errors of ``IntermediateScattering.compute``."""
        return StructureFactorResult(self._isf.compute(traj, cell, mask_a, mask_b), mask_b is None)

    def compute_for_analysis(self, la, mask_a=None, mask_b=None):
        """From the frames an analysis left resident.  ``mask_a=None``: the mobile atoms; ``mask_b``: ``None`` for the atoms of
        ``mask_a``, ``"static"`` for the static atoms of the run, else a mask or an index array."""
        if isinstance(mask_b, str):
            if mask_b != "static":
                raise ValueError("mask_b is a mask, an index array, None or \"static\"")
            _resident_columns(la, mask_a, "StructureFactor")          # has run, on one GPU
            mask_b = np.asarray(la._static_idx, dtype=np.int64)
        return StructureFactorResult(self._isf.compute_for_analysis(la, mask_a, mask_b), mask_b is None)
