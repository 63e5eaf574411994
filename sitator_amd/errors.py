"""Exception contract of the landmark path.

Same class names, attributes and messages' meaning as the reference
(``sitator/landmark/errors.py:5-40``, ``sitator/errors.py:6-21``), so ``except`` clauses and
attribute reads written against sitator keep working.
"""


class LandmarkAnalysisError(Exception):
    pass


class StaticLatticeError(LandmarkAnalysisError):
    """Static-lattice atoms moved beyond ``static_movement_threshold`` or were left unmatched.

    Attributes: ``lattice_atoms`` (indices into the static lattice), ``frame``.
    """
    TRY_RECENTERING_MSG = "Try recentering the input trajectory (sitator.util.RecenterTrajectory)"

    def __init__(self, message, lattice_atoms=None, frame=None, try_recentering=False):
        if try_recentering:
            message = message + "\n" + StaticLatticeError.TRY_RECENTERING_MSG
        super(StaticLatticeError, self).__init__(message)
        self.lattice_atoms = lattice_atoms
        self.frame = frame


class ZeroLandmarkError(LandmarkAnalysisError):
    """An all-zero landmark vector. Attributes: ``mobile_index``, ``frame``."""

    def __init__(self, mobile_index, frame):
        super(ZeroLandmarkError, self).__init__(
            "Encountered a zero landmark vector for mobile ion %i at frame %i. Try increasing "
            "`cutoff_midpoint` and/or decreasing `cutoff_steepness`." % (mobile_index, frame))
        self.mobile_index = mobile_index
        self.frame = frame


class SiteAnaysisError(Exception):
    """An error occuring as part of site analysis (spelling as in the reference)."""
    pass


class MultipleOccupancyError(SiteAnaysisError):
    """Several mobile atoms on one site in one frame. Attributes: ``mobile_particles``, ``site``, ``frame``."""

    def __init__(self, mobile, site, frame):
        super(MultipleOccupancyError, self).__init__(
            "Multiple mobile particles %s were assigned to site %i at frame %i." % (mobile, site, frame))
        self.mobile_particles = mobile
        self.site = site
        self.frame = frame


class InsufficientSitesError(SiteAnaysisError):
    """Fewer sites than mobile particles. Attributes: ``n_sites``, ``n_mobile``.

    (The reference means to raise this at ``LandmarkAnalysis.py:266-271`` but never imports the
    name, so it surfaces there as a ``NameError``; here the intended exception is raised.)"""

    def __init__(self, verb, n_sites, n_mobile):
        super(InsufficientSitesError, self).__init__(
            "%s resulted in only %i sites for %i mobile particles." % (verb, n_sites, n_mobile))
        self.n_sites = n_sites
        self.n_mobile = n_mobile


class UnassignedClampError(RuntimeError):
    """``GenerateClampedTrajectory``: a mobile atom to clamp is unassigned and ``pass_through_unassigned`` is off (the
    reference's ``RuntimeError``, ``misc/GenerateClampedTrajectory.pyx:73-74``, with its text).  Attribute:
    ``first_unassigned``, the smallest ``frame * n_mobile + mobile_atom`` of the trajectory's frames that is."""

    def __init__(self, first_unassigned):
        super(UnassignedClampError, self).__init__(
            "The mobile atoms indicated for clamping are unassigned at some point during the trajectory and "
            "`pass_through_unassigned` is set to False. Try `assign_to_last_known_site()`?")
        self.first_unassigned = first_unassigned


class VoronoiError(Exception):
    """``VoronoiSiteGenerator``: the Voronoi cell of some static atoms could not be certified, or the records could not be
    clustered into nodes unambiguously.  Attributes: ``atoms`` (static indices), ``statuses`` (per atom: 1 the search radius
    would have to grow beyond the plan, 2 a test within its error bound of a threshold, 3 a capacity of the plan exceeded),
    ``ambiguous`` (two sphere centres between 16 and 64 tolerances apart)."""

    NAMES = {1: "search radius beyond the plan", 2: "uncertain", 3: "capacity exceeded"}

    def __init__(self, atoms, statuses, ambiguous=False):
        self.atoms = [int(a) for a in atoms]
        self.statuses = [int(s) for s in statuses]
        self.ambiguous = bool(ambiguous)
        if ambiguous:
            text = "Voronoi nodes: two sphere centres lie between 16 and 64 tolerances apart; the clustering into nodes is ambiguous."
        else:
            kinds = sorted(set(self.statuses))
            text = "Voronoi nodes: %d static atoms could not be certified: %s." % (
                len(self.atoms), "; ".join("%s: atoms %s" % (self.NAMES.get(k, "status %d" % k),
                                                              [a for a, s in zip(self.atoms, self.statuses) if s == k][:16]) for k in kinds))
        super(VoronoiError, self).__init__(text)


class CoordinationEnvironmentError(Exception):
    """``SiteCoordinationEnvironment``: the Voronoi cell of some sites could not be certified.  Attributes: ``sites`` (site
    indices), ``statuses`` (per site: 1 the search radius would have to grow beyond the plan, 2 a test within its error bound
    of a threshold or an atom on the site, 3 a capacity of the plan exceeded)."""

    NAMES = VoronoiError.NAMES

    def __init__(self, sites, statuses):
        self.sites = [int(a) for a in sites]
        self.statuses = [int(s) for s in statuses]
        kinds = sorted(set(self.statuses))
        text = "Coordination environments: %d sites could not be certified: %s." % (
            len(self.sites), "; ".join("%s: sites %s" % (self.NAMES.get(k, "status %d" % k),
                                                         [a for a, s in zip(self.sites, self.statuses) if s == k][:16]) for k in kinds))
        super(CoordinationEnvironmentError, self).__init__(text)


class DeviceDomainError(Exception):
    """Internal: a domain error reported by the C-ABI before it is mapped to the classes above."""

    def __init__(self, kind, frame, index):
        super(DeviceDomainError, self).__init__("device domain error kind=%d frame=%d index=%d" % (kind, frame, index))
        self.kind = kind
        self.frame = frame
        self.index = index
