"""Shared by tests/test_hull_predicates.py (CPU) and tests/test_gpu_hull.py (GPU): a numpy restatement, written for this
project, of the gift-wrapping hull of ``k_group_hull`` (sitator_amd/csrc/hull.hip) with the rules of
sitator_amd/csrc/hull_predicates.h and the list discipline of hull_plan.h, two exact helpers on Python integers (a double is
a dyadic rational: ``fractions.Fraction`` holds it exactly), the bounds the tests use, and the designed shapes.

The restatement answers a pivot by a tournament over whole arrays (the candidate against everybody left, the first point on
its positive side takes over) where the kernel merges pairs in a tree: with certified signs both arrive at the same winner,
and the facets then come in the same order.  Where a sign is not certified the two may look at different pairs, so which
sites are flagged is compared only on shapes designed to be degenerate."""
from fractions import Fraction

import numpy as np

from tests import group_ref as GR

POS, NEG, UNCERTAIN = 1, -1, 0
CLOSED, FEW, FLAGGED, CAPACITY, OPEN = 0, 1, 2, 3, 4
FACET_CAP = 2048                                   # HP_FACET_CAP; the tests compare it with sit_hull_plan
EPS = 2.0 ** -53
BOUND_A = (7.0 + 56.0 * EPS) * EPS

# ``scipy.spatial.ConvexHull(...).volume`` against the exact volume of the wrap's facets, the largest relative difference
# over every input of the two test files (each site and step of the goldens, every designed shape): measured 6.97e-14, on a
# 4-point site of the "large" grouping (a tetrahedron of size 1 that the recentring puts at coordinates around 32; the
# goldens' largest is 1.6e-15, the wrap's own 4.7e-16; tests/test_hull_predicates.py prints them).  qhull merges nearly
# coplanar facets under a tolerance of its own, so this is not derivable; 64 times the measured value is allowed.
QHULL_MEASURED_REL = 7.0e-14
QHULL_REL_TOL = 64 * QHULL_MEASURED_REL

CELL = np.eye(3) * 64.0                            # a power of two: shifting and wrapping dyadic coordinates is exact


# ---- the predicate ------------------------------------------------------------------------------------------------------------

def det_permanent(a, b, c, q):
    """(D, permanent) in double, in the operation order of hp_det; ``q`` may be an array [n, 3]."""
    a, b, c, q = (np.asarray(x, dtype=np.float64) for x in (a, b, c, q))
    adx, bdx, cdx = a[..., 0] - q[..., 0], b[..., 0] - q[..., 0], c[..., 0] - q[..., 0]
    ady, bdy, cdy = a[..., 1] - q[..., 1], b[..., 1] - q[..., 1], c[..., 1] - q[..., 1]
    adz, bdz, cdz = a[..., 2] - q[..., 2], b[..., 2] - q[..., 2], c[..., 2] - q[..., 2]
    bdxcdy, cdxbdy = bdx * cdy, cdx * bdy
    cdxady, adxcdy = cdx * ady, adx * cdy
    adxbdy, bdxady = adx * bdy, bdx * ady
    det = adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy) + cdz * (adxbdy - bdxady)
    permanent = ((np.abs(bdxcdy) + np.abs(cdxbdy)) * np.abs(adz) + (np.abs(cdxady) + np.abs(adxcdy)) * np.abs(bdz)
                 + (np.abs(adxbdy) + np.abs(bdxady)) * np.abs(cdz))
    return det, permanent


def orient(a, b, c, q):
    """hp_orient3d: POS where D < -bound, NEG where D > bound, UNCERTAIN otherwise."""
    det, permanent = det_permanent(a, b, c, q)
    bound = BOUND_A * permanent
    return np.where(det > bound, NEG, np.where(-det > bound, POS, UNCERTAIN))


def exact_det(a, b, c, q):
    """D = det [a - q; b - q; c - q] as a Fraction, no rounding anywhere."""
    r = [[Fraction(float(p[d])) - Fraction(float(q[d])) for d in range(3)] for p in (a, b, c)]
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = r
    return az * (bx * cy - cx * by) + bz * (cx * ay - ax * cy) + cz * (ax * by - bx * ay)


def exact_orient(a, b, c, q):
    d = exact_det(a, b, c, q)
    return POS if d < 0 else NEG if d > 0 else UNCERTAIN


def exact_volume(points, facets):
    """The volume enclosed by the facet list (tetrahedra against the first facet's first vertex), as a Fraction."""
    if len(facets) == 0:
        return Fraction(0)
    p0 = points[facets[0][0]]
    return sum((exact_det(points[u], points[v], points[w], p0) for u, v, w in facets), Fraction(0)) / 6


def volume_bound(points, facets):
    """|the kernel's volume - the exact volume of its own facet list| <= 2^-53 (8 sum permanent_i + F sum |det_i|) / 6: a
    facet's determinant is within (7 + 56 eps) eps of its permanent, a sum of F terms in any order within F eps of the sum
    of their magnitudes (the division by 6 is one more rounding of the total, inside the same term)."""
    facets = np.asarray(facets).reshape(-1, 3)
    if len(facets) == 0:
        return 0.0
    p0 = points[facets[0, 0]]
    det, permanent = det_permanent(points[facets[:, 0]], points[facets[:, 1]], points[facets[:, 2]], p0)
    return EPS * (8.0 * float(np.sum(permanent)) + len(facets) * float(np.sum(np.abs(det)))) / 6.0


# ---- the wrap -----------------------------------------------------------------------------------------------------------------

def _same(P, p):
    return (P[:, 0] == p[0]) & (P[:, 1] == p[1]) & (P[:, 2] == p[2])


def pivot(P, pa, pb, b_real):
    """(winner or None, uncertain): the point no other point is POS of (pa, pb, .); of equal points the lowest index."""
    keep = ~_same(P, pa)
    if b_real:
        keep &= ~_same(P, pb)
    rest = np.nonzero(keep)[0]
    if len(rest) == 0:
        return None, False
    c, rest, uncertain = int(rest[0]), rest[1:], False
    while len(rest):
        rest = rest[~_same(P[rest], P[c])]
        s = orient(pa, pb, P[c], P[rest])
        uncertain = uncertain or bool(np.any(s == UNCERTAIN))
        rest = rest[s == POS]
        if len(rest):
            c, rest = int(rest[0]), rest[1:]
    return c, uncertain


def wrap(points, facet_cap=FACET_CAP):
    """{'status', 'facets' [F, 3] in the order found, 'vertices' (sorted), 'volume' (double, summed in that order; NaN unless
    closed)} of one site."""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    out = {"status": None, "facets": np.zeros((0, 3), dtype=np.int64), "vertices": np.zeros(0, dtype=np.int64), "volume": np.nan}
    if len(P) < 4:
        out["status"] = FEW
        return out
    order = np.lexsort((np.arange(len(P)), P[:, 2], P[:, 1], P[:, 0]))
    a = int(order[0])
    b, unc = pivot(P, P[a], P[a] + np.array([0.0, 1.0, 0.0]), False)
    if b is None or unc:
        out["status"] = FLAGGED
        return out
    c, unc = pivot(P, P[a], P[b], True)
    if c is None or unc:
        out["status"] = FLAGGED
        return out
    facets, open_, seen = [(a, b, c)], [(b, a), (c, b), (a, c)], {a, b, c}
    vol = float(det_permanent(P[a], P[b], P[c], P[a])[0])
    status = None
    while status is None:
        if len(open_) > facet_cap + 2:
            status = CAPACITY
        elif not open_:
            F, V = len(facets), len(seen)
            status = CLOSED if F % 2 == 0 and V - 3 * (F // 2) + F == 2 else OPEN
        elif len(facets) >= facet_cap:
            status = CAPACITY
        else:
            u, v = open_.pop()
            w, unc = pivot(P, P[u], P[v], True)
            if w is None or unc:
                status = FLAGGED
                break
            p1 = open_.index((v, w)) if (v, w) in open_ else -1
            p2 = open_.index((w, u)) if (w, u) in open_ else -1
            for p in sorted((p1, p2), reverse=True):
                if p >= 0:
                    last = open_.pop()
                    if p < len(open_):
                        open_[p] = last
            if p1 < 0:
                open_.append((w, v))
            if p2 < 0:
                open_.append((u, w))
            facets.append((u, v, w))
            seen.add(w)
            vol = vol + float(det_permanent(P[u], P[v], P[w], P[a])[0])
    out["status"] = status
    out["facets"] = np.array(facets, dtype=np.int64)
    out["vertices"] = np.array(sorted(seen), dtype=np.int64)
    if status == CLOSED:
        out["volume"] = vol / 6.0
    return out


def qhull(points):
    """(vertices sorted, volume) of scipy's hull; (None, None) where qhull refuses."""
    from scipy.spatial import ConvexHull
    try:
        from scipy.spatial import QhullError
    except ImportError:                                            # scipy < 1.8
        from scipy.spatial.qhull import QhullError
    try:
        h = ConvexHull(points)
    except QhullError:
        return None, None
    return np.sort(h.vertices), float(h.volume)


# ---- designed shapes ----------------------------------------------------------------------------------------------------------

def gaussian(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3))


def uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3))


def shell(n, seed):
    """n points on the unit sphere (to rounding): every one is a vertex, 2 n - 4 facets."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.sqrt(np.sum(v * v, axis=1))[:, None]


CUBE = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
THREE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.25]])


def coplanar(n, seed):
    """n points with dyadic coordinates in the plane z = 1 / 2."""
    p = np.random.default_rng(seed).integers(-512, 512, size=(n, 3)) / 256.0
    p[:, 2] = 0.5
    return p


def interior5(seed):
    """A tetrahedron and a point inside it."""
    p = gaussian(4, seed)
    return np.concatenate([p, p.mean(axis=0)[None]])


# (name, sites): every site a (kind, n, seed).  A seed is kept if the restatement's vertex set equals scipy's on the
# recentred copy of the site, and stepped otherwise; none of the seeds below had to be stepped, and the tests assert the
# agreement again.  The lengths are the edges of the lane, wave and workgroup trees of the reduction.
GROUPINGS = {
    "edges": [("gaussian", 4, 0), ("interior5", 5, 0), ("uniform", 63, 0), ("gaussian", 64, 0), ("uniform", 65, 0),
              ("gaussian", 255, 0), ("uniform", 256, 0), ("gaussian", 257, 0), ("uniform", 1025, 0)],
    "large": [("gaussian", 4, 1), ("gaussian", 20000, 0), ("gaussian", 4, 2)],
    "many": [("gaussian", 8, s) for s in range(600)],
    "shell": [("shell", 600, 0)],
    "doubled": [("doubled", 130, 0), ("doubled", 8, 1)],
    "small": [("gaussian", 4, 3), ("interior5", 5, 1), ("gaussian", 4, 4)],            # 3 sites over 13 points
}
FLAGGED_SITES = [("cube", 8, 0, FLAGGED), ("three", 3, 0, FEW), ("coplanar", 40, 0, FLAGGED), ("shell", 1100, 1, CAPACITY)]


def cloud(kind, n, seed):
    if kind == "gaussian":
        return gaussian(n, seed)
    if kind == "uniform":
        return uniform(n, seed)
    if kind == "shell":
        return shell(n, seed)
    if kind == "interior5":
        return interior5(seed)
    if kind == "doubled":                                          # every point stored twice, the copies shuffled in
        p = gaussian(n // 2, seed)
        return np.concatenate([p, p])[np.random.default_rng(seed + 7).permutation(2 * (n // 2))]
    if kind == "cube":
        return CUBE.copy()
    if kind == "three":
        return THREE.copy()
    if kind == "coplanar":
        return coplanar(n, seed)
    raise ValueError(kind)


def grouping(sites, cell=CELL):
    """(labels [F, 1], positions [F, 1, 3], offsets [K + 1], working copy [N, 3] after step 0 of one recentring) of one ion
    that visits the sites in turn: site s holds the points of ``sites[s]`` in order."""
    clouds = [cloud(*s[:3]) for s in sites]
    labels = np.concatenate([np.full(len(c), k, dtype=np.int64) for k, c in enumerate(clouds)]).reshape(-1, 1)
    pos = np.concatenate(clouds).reshape(-1, 1, 3)
    off, _, pts, _ = GR.grouped(labels, len(sites), pos, np.arange(1))
    work = next(GR.recenter_steps(cell, off, pts, 1))
    return labels, pos, off, work


def golden_sites():
    """Yields (name, step count, step, site, points) over every site and step of the goldens' out_recentered_r1 / r8."""
    GG = GR.GroupGoldens()
    for name in GG.names:
        off = GG.get(name, "out_offsets")
        for nr in (1, 8):
            rec = GG.get(name, "out_recentered_r%d" % nr)
            for i in range(nr):
                for s in range(len(off) - 1):
                    yield name, nr, i, s, rec[i, off[s]:off[s + 1]]
