"""``VoronoiSiteGenerator`` (reference: ``sitator/voronoi.py``): the Voronoi nodes of the static lattice as landmark sites.

The reference writes the static structure to a file and runs the external Zeo++ ``network`` binary (``sitator/util/zeo.py``).
Here the periodic Voronoi nodes come from ``sit_voronoi_nodes`` (``csrc/voronoi.hip``, every decision in
``csrc/voronoi_plan.h``): a neighbour kernel and a sphere kernel, one workgroup per atom, and a merge of the records into
nodes.  There is no CPU fallback, as everywhere else.

A node is a sphere ``(c, r)`` with no atom image closer to ``c`` than ``r - tolerance`` and at least four atom images, not
coplanar, within ``tolerance`` of the sphere; its vertices are the static indices (statics-only numbering, what
``LandmarkAnalysis`` reads) of all atom images on it, unique and ascending.  One degenerate sphere - the 8 atoms about the centre
of a simple-cubic cube, the 6 about an FCC octahedral hole - is one node with all of its atoms, as Zeo++ reports it.  In a cell
so small that images of one atom share a sphere a node has fewer than 4 unique vertices.
"""
import numpy as np

from . import _lib
from .errors import VoronoiError
from .site_network import SiteNetwork


class VoronoiSiteGenerator(object):
    """Given an empty ``SiteNetwork``, use the Voronoi decomposition of its static lattice to generate sites.

    :param bool radial: the radical (radius-weighted) tessellation.  Not implemented: it needs atomic radii, which a
        ``SiteNetwork`` does not carry.
    :param float tolerance: ``tau`` in Angstrom: how far from a sphere an atom still counts as on it.
    :param str zeopp_path: accepted for source compatibility with the reference and ignored.
    :param int device: the GPU.
    """

    def __init__(self, radial=False, tolerance=1e-6, zeopp_path=None, device=0):
        if radial:
            raise NotImplementedError("VoronoiSiteGenerator: the radical tessellation needs atomic radii, which are not carried")
        if not tolerance > 0.0:
            raise ValueError("VoronoiSiteGenerator: the tolerance must be positive")
        self._tolerance = float(tolerance)
        self._device = int(device)
        self.last_info = None

    def run(self, sn):
        """``sn.copy()`` with ``centers`` set to the Voronoi nodes of ``sn.static_structure`` (wrapped into the cell) and
        ``vertices`` to a list of lists of static indices.  Any atom whose cell could not be certified raises
        ``VoronoiError``: a partial network is never returned."""
        assert isinstance(sn, SiteNetwork)
        static = sn.static_structure
        positions = np.ascontiguousarray(static.get_positions(), dtype=np.float64)
        cell = np.asarray(static.cell, dtype=np.float64).reshape(3, 3)
        with _lib.HipContext(cell, device=self._device) as ctx:
            res = ctx.voronoi_nodes(positions, self._tolerance)
        self.last_info = res["info"]
        bad = np.nonzero(res["status"] != 0)[0]
        if len(bad):
            raise VoronoiError(bad, res["status"][bad])
        if res["info"]["merge_status"] != 0:
            raise VoronoiError([], [], ambiguous=True)
        out = sn.copy()
        out.centers = res["centers"]
        out.vertices = [[int(i) for i in v] for v in res["vertices"]]
        return out
