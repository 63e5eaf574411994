"""``sitator.network`` on the device: ``DiffusionPathwayAnalysis`` (``network/DiffusionPathwayAnalysis.py``), the step after
``JumpAnalysis`` that says which sites form pathways crossing the periodic cell, and ``MergeSitesByBarrier``
(``network/MergeSitesByBarrier.py``), which merges sites that a low energy barrier separates (at the end of this file).

The reference builds the graph of the 3 x 3 x 3 supercell with one Python call per edge per image and hands it to scipy.  Here
the image code of every connected pair, the edge list and the connected components of the 27 K nodes come from
``sit_pathway_components`` (``csrc/pathways.hip``, decisions in ``csrc/pathway_graph.h``); the host thresholds ``n_ij`` with
numpy exactly as the reference does, ranks the component roots and does the per-component bookkeeping, which is small.
"""
import itertools
import logging
import numbers

import numpy as np

from . import _lib
from .calculators import LennardJones
from .merging import MergeSites
from .pbc import PBCCalculator

logger = logging.getLogger(__name__)

# the images of the supercell in node order: node = image * K + site
IMAGES = np.array(list(itertools.product(range(-1, 2), repeat=3)), dtype=np.int64)
HOME_IMAGE = 13
assert tuple(IMAGES[HOME_IMAGE]) == (0, 0, 0)


def home_nodes(n_sites):
    """The nodes a component must touch to be looked at.  The reference marks ``mask_000[13:13 + n_sites]``
    (``DiffusionPathwayAnalysis.py:189-192``: the home image's index is not multiplied by the number of sites), so these are
    the nodes 13 ... 13 + n_sites - 1 of the supercell and not the n_sites nodes of image 13.  That decides which components
    become pathways and in which order they are numbered, so it is kept as it is: results are the reference's."""
    return slice(HOME_IMAGE, HOME_IMAGE + int(n_sites))


def rank_roots(root):
    """Component numbers from ``root`` (per node the lowest node index of its component): the components numbered in the order
    of their lowest node, which is how ``scipy.sparse.csgraph.connected_components`` numbers them."""
    return np.unique(np.asarray(root), return_inverse=True)[1].reshape(-1).astype(np.int64)


def periodic_pathways(labels, n_sites):
    """The bookkeeping of ``DiffusionPathwayAnalysis.py:82-143`` on the component numbers ``labels`` ``[27 * n_sites]`` of the
    supercell graph: ``(site_pathway [n_sites], directions)`` - per site its pathway or -1, and per pathway the set of
    direction triples.  Components are visited in ascending number; one that does not touch ``home_nodes`` or holds no site
    twice is passed over; the others claim their sites, absorbing every earlier pathway they share a site with."""
    K = int(n_sites)
    labels = np.asarray(labels).reshape(27, K)
    order = np.argsort(labels, axis=None, kind="stable")         # nodes grouped by component, ascending inside one
    sorted_labels = labels.reshape(-1)[order]
    starts = np.flatnonzero(np.r_[True, sorted_labels[1:] != sorted_labels[:-1]])
    ends = np.r_[starts[1:], len(order)]
    begin_of = dict(zip(sorted_labels[starts].tolist(), zip(starts.tolist(), ends.tolist())))
    claimed = np.zeros(K, dtype=np.int64)                        # 0: by nobody; else the stamp of the live pathway
    live = {}                                                    # stamp -> (sites, directions), in order of creation
    stamp = 1
    for comp in np.unique(labels.reshape(-1)[home_nodes(K)]).tolist():   # (no other component changes anything)
        lo, hi = begin_of[comp]
        nodes = order[lo:hi]
        if hi - lo < 2:
            continue
        site, image = nodes % K, nodes // K
        by_site = np.lexsort((image, site))
        site, image = site[by_site], image[by_site]
        first = np.flatnonzero(np.r_[True, site[1:] != site[:-1]])
        twice = first[np.diff(np.r_[first, len(site)]) > 1]
        if twice.size == 0:
            continue                                             # it does not reach an image of one of its own sites
        # the direction between the first two images of every site that is there twice (:108-113)
        crossing = (IMAGES[image[twice]] - IMAGES[image[twice + 1]]) != 0
        directions = set(tuple(row) for row in crossing)
        sites = site[first]
        met = np.unique(claimed[sites])
        for old in met[met > 0].tolist():
            old_sites, old_directions = live.pop(old)
            sites = np.union1d(sites, old_sites)
            directions |= old_directions
        live[stamp] = (sites, directions)
        claimed[sites] = stamp
        stamp += 1
    site_pathway = np.full(K, DiffusionPathwayAnalysis.NO_PATHWAY, dtype=np.int64)
    for number, (sites, _) in enumerate(live.values()):
        site_pathway[sites] = number
    return site_pathway, [d for _, d in live.values()]


class DiffusionPathwayAnalysis(object):
    """Find connected diffusion pathways in a ``SiteNetwork`` (``sitator.network.DiffusionPathwayAnalysis``).

    :param float|int connectivity_threshold: an integer is the number of jumps an edge needs to count as connected, a real
        the fraction of all jumps between different sites.
    :param bool true_periodic_pathways: keep only pathways that contain a site AND one of its periodic images, i.e. that
        conduct through the bulk; ``minimum_n_sites`` is then not looked at.  Otherwise every connected component of at least
        ``minimum_n_sites`` sites is a pathway.
    :param int minimum_n_sites: see above.

    One deliberate departure from the reference: ``run(..., return_direction=True)`` with ``true_periodic_pathways=False``
    raises ``ValueError`` before anything is computed; the reference fails there with ``UnboundLocalError`` after it has
    added its attributes (directions exist for periodic pathways only).
    """

    NO_PATHWAY = -1

    def __init__(self, connectivity_threshold=1, true_periodic_pathways=True, minimum_n_sites=0):
        assert minimum_n_sites >= 0
        self.true_periodic_pathways = true_periodic_pathways
        self.connectivity_threshold = connectivity_threshold
        self.minimum_n_sites = minimum_n_sites
        self.rounds = None                                       # rounds the device labelling of the last run took
        self._ctx, self._ctx_cell = None, None

    def _device(self, cell):
        cell = np.array(cell, dtype=np.float64).reshape(3, 3)
        if self._ctx is None or not np.array_equal(cell, self._ctx_cell):
            self._ctx, self._ctx_cell = _lib.HipContext(cell), cell
        return self._ctx

    def connectivity_matrix(self, n_ij):
        """``(n_ij >= threshold, threshold, number of jumps between different sites)`` (:60-71)."""
        n_ij = np.asarray(n_ij)
        off_diagonal = np.ones(shape=n_ij.shape, dtype=bool)
        np.fill_diagonal(off_diagonal, False)
        n_non_self_jumps = np.sum(n_ij[off_diagonal])
        if isinstance(self.connectivity_threshold, numbers.Integral):
            threshold = self.connectivity_threshold
        elif isinstance(self.connectivity_threshold, numbers.Real):
            threshold = self.connectivity_threshold * n_non_self_jumps
        else:
            raise TypeError("Don't know how to interpret connectivity_threshold `%s`" % self.connectivity_threshold)
        return n_ij >= threshold, threshold, n_non_self_jumps

    def run(self, sn, return_count=False, return_direction=False):
        """Expects a ``SiteNetwork`` that a ``JumpAnalysis`` has run on; adds ``site_diffusion_pathway`` (per site its
        pathway, ``NO_PATHWAY`` for none) and ``edge_diffusion_pathway`` (per pair the pathway both belong to) to it.

        Returns ``(sn, [number of pathways], [per pathway a set of direction triples])``: a triple says along which cell
        vectors the pathway joins a site to its periodic image.
        """
        if not sn.has_attribute('n_ij'):
            raise ValueError("SiteNetwork has no `n_ij`; run a JumpAnalysis on it first.")
        if return_direction and not self.true_periodic_pathways:
            raise ValueError("`return_direction` needs `true_periodic_pathways`: only periodic pathways have directions.")
        connected, threshold, n_non_self_jumps = self.connectivity_matrix(sn.n_ij)
        K = sn.n_sites
        assert connected.shape == (K, K)
        n_images = 27 if self.true_periodic_pathways else 1
        root, self.rounds, _ = self._device(sn.structure.cell).pathway_components(connected, sn.centers, n_images)
        labels = rank_roots(root)
        directions = None
        if self.true_periodic_pathways:
            site_pathway, directions = periodic_pathways(labels, K)
        else:
            sizes = np.bincount(labels, minlength=0)
            is_pathway = sizes >= self.minimum_n_sites
            number = np.full(len(sizes), self.NO_PATHWAY, dtype=np.int64)
            number[is_pathway] = np.arange(np.count_nonzero(is_pathway))
            site_pathway = number[labels]
            logger.info("Taking all edges with at least %s/%s jumps..." % (threshold, n_non_self_jumps))
            logger.info("Found %i connected components, of which %i are large enough to qualify as pathways (%i sites)."
                        % (len(sizes), np.count_nonzero(is_pathway), self.minimum_n_sites))
        n_pathways = int(site_pathway.max()) + 1 if K else 0
        together = site_pathway[:, None] == site_pathway[None, :]
        edge_pathway = np.where(together, site_pathway[:, None], self.NO_PATHWAY)
        sn.add_site_attribute('site_diffusion_pathway', site_pathway)
        sn.add_edge_attribute('edge_diffusion_pathway', edge_pathway)
        out = [sn]
        if return_count:
            out.append(n_pathways)
        if return_direction:
            out.append(directions)
        return tuple(out)


class MergeSitesByBarrier(MergeSites):
    """Merge sites based on the energy barrier between them (``sitator.network.MergeSitesByBarrier``).

    For every pair of sites within ``maximum_pairwise_distance`` that exchanged at least ``minimum_jumps_mergable`` jumps, one
    mobile atom is driven in ``n_driven_images`` evenly spaced steps along the straight line from one centre to the nearest
    image of the other, in the frozen lattice of the atoms of ``coordinating_mask`` (default: the static atoms).  If the highest
    image is neither end of the path, the pair is mergable from i to j when that image lies at most ``barrier_threshold`` above
    the first one, and from j to i when it lies at most ``barrier_threshold`` above the last one; if it is an end, the two sites
    share a basin and the pair stays as the distance and the jump counts left it.  The strongly connected components of the
    mergable matrix are merged (further keywords go to ``MergeSites``).

    :param calculator: a ``sitator_amd.calculators.LennardJones``.
    :param float barrier_threshold: the barrier above which two sites are not mergable (units of ``epsilon``).
    :param int n_driven_images: at least 3.
    :param float maximum_pairwise_distance, maximum_merge_distance: Angstrom.
    :param int minimum_jumps_mergable: compared with ``n_ij``.

    All image energies of all pairs come from one call of ``sit_barrier_energies`` (``csrc/barrier.hip``); they hold the mobile
    atom's energy only - the energy of the lattice with itself, which the reference's calculator includes in every total, is
    the same for all images and drops out of both barriers.  After ``run()`` the operator keeps ``pairs_`` ``[P, 2]`` (i < j, in
    the reference's order), ``energies_`` ``[P, n_driven_images]`` and ``mergable_`` ``[K, K]``, the matrix handed to
    ``connected_components``.

    Deliberate departures from the reference:

    * ``calculator`` is not an arbitrary ASE calculator: anything but a ``LennardJones`` raises ``TypeError``.  The energies
      are evaluated on the device and there is no CPU fallback.
    * Without ``n_ij`` on the network a ``JumpAnalysis`` is run first.  The reference means to (:72-74) but never imports
      ``JumpAnalysis`` and ends in ``NameError``.
    """

    def __init__(self, calculator, barrier_threshold, n_driven_images=20, maximum_pairwise_distance=2, minimum_jumps_mergable=1,
                 maximum_merge_distance=2, **kwargs):
        super(MergeSitesByBarrier, self).__init__(maximum_merge_distance=maximum_merge_distance, **kwargs)
        if not isinstance(calculator, LennardJones):
            raise TypeError("MergeSitesByBarrier: `calculator` must be a sitator_amd.calculators.LennardJones, not %s: the "
                            "energies are evaluated on the device and there is no CPU fallback" % type(calculator).__name__)
        self.barrier_threshold = barrier_threshold
        self.maximum_pairwise_distance = maximum_pairwise_distance
        self.minimum_jumps_mergable = minimum_jumps_mergable
        assert n_driven_images >= 3, "Must have at least initial, transition, and final."
        self.n_driven_images = n_driven_images
        self.calculator = calculator
        self.pairs_ = self.energies_ = self.mergable_ = None

    def _get_sites_to_merge(self, st, coordinating_mask=None):
        from scipy.sparse.csgraph import connected_components
        sn = st.site_network
        if not sn.has_attribute('n_ij'):                         # :72-74
            from .dynamics import JumpAnalysis
            JumpAnalysis().run(st)
        pos = np.asarray(sn.centers, dtype=np.float64)
        if coordinating_mask is None:                            # :77-80
            coordinating_mask = sn.static_mask
        else:
            coordinating_mask = np.asarray(coordinating_mask, dtype=bool)
            assert not np.any(coordinating_mask & sn.mobile_mask)
        static_pos = np.asarray(sn.structure.get_positions(), dtype=np.float64)[coordinating_mask]
        eps, sigma = self.calculator.parameters_for(np.asarray(sn.structure.get_atomic_numbers())[coordinating_mask])
        interpolation_coeffs = np.linspace(0, 1, self.n_driven_images)   # :87

        # -- Decide on pairs to check (:90-101)
        pbcc = PBCCalculator(np.asarray(sn.structure.cell, dtype=np.float64))
        dists = pbcc.pairwise_distances(pos)
        mergable = dists <= self.maximum_pairwise_distance
        mergable &= np.asarray(sn.n_ij) >= self.minimum_jumps_mergable
        first, second = np.nonzero(np.triu(mergable | mergable.T, k=1))   # the order of itertools.combinations
        pairs = np.stack([first, second], axis=1).astype(np.int32)

        # -- Check pairs' barriers (:103-125)
        energies, verdict, _ = pbcc._ctx.barrier_energies(static_pos, eps, sigma, self.calculator.rc, pos, pairs,
                                                          interpolation_coeffs, self.barrier_threshold)
        interior = verdict[:, 0] != 0
        mergable[first[interior], second[interior]] = verdict[interior, 1] != 0
        mergable[second[interior], first[interior]] = verdict[interior, 2] != 0
        self.pairs_, self.energies_, self.mergable_ = pairs, energies, mergable.copy()

        n_merged_sites, labels = connected_components(mergable, directed=True, connection='strong')   # :128-132
        return [np.where(labels == lbl)[0] for lbl in range(n_merged_sites)]
