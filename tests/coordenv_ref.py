"""numpy / scipy restatement of SiteCoordinationEnvironment (sitator_amd/csrc/coordenv_plan.h), written
independently of the header: the site's Voronoi cell comes from qhull (``scipy.spatial.Voronoi`` over the site and the static
images within the search radius), the solid angle of a face from a fan about its first vertex, the shape measure from
``itertools.permutations`` and ``numpy.linalg.svd``.  The shape library is typed in here a second time, from rings and signs
rather than from the header's closed forms.  Agreement with a pymatgen installation is not claimed; the yardsticks are the closed-form values below.

``MEASURED`` is the largest absolute deviation between the device and this restatement over the fixtures (csm on its 0 - 100
scale, confidence, normalised distance and angle), ``TOL`` 64 times it - the rule of ``voronoi_ref.CENTER_TOL``."""
import functools
import itertools

import numpy as np

from tests import barrier_ref as BR
from tests import voronoi_ref as VR

OK, GROW, UNCERTAIN, CAPACITY = 0, 1, 2, 3
NEAR_CUTOFF = 1
TAU = 1e-6
DISTANCE_CUTOFF, ANGLE_CUTOFF, MAX_CSM = 1.4, 0.3, 8.0
SYMBOLS = ("S:1", "L:2", "TL:3", "T:4", "S:4", "T:5", "S:5", "O:6", "T:6", "PB:7", "C:8", "SA:8")
MEASURED = 3.56e-13    # fcc_jitter, a shape measure; the host probe of tests/test_coordenv_plan.py deviates by the same
TOL = 64 * MEASURED
SELECT_MARGIN = 1e-3   # every coordinating decision of a fixture is at least this far (relative) from its cutoff
SHAPE_MARGIN = 1e-6    # every best-shape decision has at least this gap in S to the runner-up


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=1)[:, None]


def _ring(n, z=0.0, r=1.0, phase=0.0):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([r * np.cos(a), r * np.sin(a), np.full(n, z)], axis=1)


@functools.lru_cache(maxsize=None)
def shapes():
    """symbol -> [n, 3] unit vertices, library order."""
    out = {}
    out["S:1"] = np.array([[0.0, 0.0, 1.0]])
    out["L:2"] = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    out["TL:3"] = _ring(3)
    out["T:4"] = _unit([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    out["S:4"] = _ring(4)
    out["T:5"] = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0]], _ring(3)])
    out["S:5"] = np.concatenate([[[0, 0, 1.0]], _ring(4)])
    out["O:6"] = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    r = 1.0
    out["T:6"] = _unit(np.concatenate([_ring(3, r * np.sqrt(3.0) / 2.0, r), _ring(3, -r * np.sqrt(3.0) / 2.0, r)]))
    out["PB:7"] = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0]], _ring(5)])
    out["C:8"] = _unit([[x, y, z] for z in (1, -1) for y in (1, -1) for x in (1, -1)])
    a = 1.0
    sep = a * 2.0 ** -0.25
    out["SA:8"] = _unit(np.concatenate([_ring(4, sep / 2.0, a / np.sqrt(2.0)), _ring(4, -sep / 2.0, a / np.sqrt(2.0), np.pi / 4.0)]))
    assert tuple(out) == SYMBOLS
    return out


def shapes_of(n):
    return [s for s in SYMBOLS if len(shapes()[s]) == n]


@functools.lru_cache(maxsize=None)
def _perms(n):
    return np.array(list(itertools.permutations(range(n))), dtype=np.int64)


def csm(q, p):
    """100 * min over assignments, proper rotations and scales of sum |q_k - s R p_pi(k)|^2 / sum |q_k|^2, by the singular values of
    M = sum q_k p_pi(k)^T: t = s1 + s2 + sign(det M) s3."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n = len(q)
    assert len(p) == n
    if n == 1:
        return 0.0
    best = -np.inf
    perms = _perms(n)
    for lo in range(0, len(perms), 8192):
        pp = p[perms[lo:lo + 8192]]                                   # [m, n, 3]
        M = np.einsum("ka,mkb->mab", q, pp)
        sv = np.linalg.svd(M, compute_uv=False)
        sign = np.where(np.linalg.det(M) < 0.0, -1.0, 1.0)
        best = max(best, float((sv[:, 0] + sv[:, 1] + sign * sv[:, 2]).max()))
    return max(0.0, 100.0 * (1.0 - best * best / (float((q * q).sum()) * float((p * p).sum()))))


def weight(S, max_csm=MAX_CSM):
    return (1.0 - S / max_csm) ** 2 if S < max_csm else 0.0


def decide(n, q, max_csm=MAX_CSM):
    """``(symbol, csm_best, csm_all [3] NaN padded, confidence, gap to the runner-up)`` of n coordinating images q."""
    all3 = np.full(3, np.nan)
    if n == 0:
        return "BAD:0", np.nan, all3, 0.0, np.inf
    names = shapes_of(n) if n <= 8 else []
    vals = [csm(q, shapes()[s]) for s in names]
    all3[:len(vals)] = vals
    if not names:
        return "UN:%d" % n, np.nan, all3, 0.0, np.inf
    best = int(np.argmin(vals))
    gap = min([abs(v - vals[best]) for j, v in enumerate(vals) if j != best] + [abs(max_csm - vals[best])])
    w = [weight(v, max_csm) for v in vals]
    if not vals[best] < max_csm:
        return "UN:%d" % n, vals[best], all3, 0.0, gap
    return names[best], vals[best], all3, w[best] / sum(w), gap


def site_neighbours(cell, pos, c, R):
    """Every static image within R of the point c, relative to it, ordered by (squared distance, static index, image): the
    arithmetic of ``voronoi_ref.neighbours`` with a site in the atom's place."""
    cell, pos, c = np.asarray(cell, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(c, dtype=np.float64)
    ci = VR.cell_inverse(cell)
    h = BR.heights(cell)
    g = (c[None, :] - pos) @ ci.T
    reach = np.ceil(R / h) + 1
    lo = np.floor(g.min(axis=0) - reach).astype(np.int64)
    hi = np.ceil(g.max(axis=0) + reach).astype(np.int64)
    m = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    mf = m.astype(np.float64)
    T = np.stack([(mf[:, 0] * cell[0, k] + mf[:, 1] * cell[1, k]) + mf[:, 2] * cell[2, k] for k in range(3)], axis=1)
    out_q, out_s, out_m, out_d = [], [], [], []
    for s in range(len(pos)):
        d = (c - pos[s])[None, :] - T
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 <= R * R
        if keep.any():
            out_q.append(-d[keep]); out_m.append(m[keep]); out_d.append(d2[keep]); out_s.append(np.full(int(keep.sum()), s))
    if not out_q:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int64)
    q, m, d2, s = np.concatenate(out_q), np.concatenate(out_m), np.concatenate(out_d), np.concatenate(out_s)
    order = np.lexsort((m[:, 2], m[:, 1], m[:, 0], s, d2))
    return q[order], s[order].astype(np.int64)


def triangle_angle(a, b, c):
    """Van Oosterom & Strackee: the signed solid angle of the triangle (a, b, c) from the origin."""
    la, lb, lc = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)
    return 2.0 * np.arctan2(np.dot(a, np.cross(b, c)), la * lb * lc + np.dot(a, b) * lc + np.dot(a, c) * lb + np.dot(b, c) * la)


def polygon_angle(verts, normal):
    """The solid angle from the origin of the convex polygon with these vertices in the plane of this normal."""
    verts = np.asarray(verts, dtype=np.float64)
    if len(verts) < 3:
        return 0.0
    mean = verts.mean(axis=0)
    e1 = np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 * np.linalg.norm(normal) else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal / np.linalg.norm(normal), e1)
    d = verts - mean
    order = np.argsort(np.arctan2(d @ e2, d @ e1), kind="stable")
    v = verts[order]
    return abs(sum(triangle_angle(v[0], v[k], v[k + 1]) for k in range(1, len(v) - 1)))


def site_round(q, R):
    """The site's cell among the neighbours q within R: ``None`` when it is not complete at R (an empty open octant, an unbounded
    cell, or a cell vertex farther than R / 2), else ``{neighbour position: solid angle}`` of its faces."""
    from scipy.spatial import Voronoi
    if len(q) < 4 or VR.octants(q) != 0xFF:
        return None
    vor = Voronoi(np.concatenate([np.zeros((1, 3)), q]))
    region = vor.regions[vor.point_region[0]]
    if -1 in region or len(region) == 0:
        return None
    if np.linalg.norm(vor.vertices[region], axis=1).max() > 0.5 * R:
        return None
    faces = {}
    for (a, b), rv in zip(vor.ridge_points, vor.ridge_vertices):
        if a != 0 and b != 0:
            continue
        j = int(max(a, b)) - 1
        faces[j] = polygon_angle(vor.vertices[rv], q[j])
    return faces


def site(cell, pos, c, distance_cutoff=DISTANCE_CUTOFF, angle_cutoff=ANGLE_CUTOFF, max_csm=MAX_CSM):
    """The whole answer for one site: a dict of ``rounds``, ``n``, ``vertices`` (static indices in order), ``norm_distance``,
    ``norm_angle``, ``symbol``, ``csm_best``, ``csm_all``, ``confidence`` and the two margins (``select_margin``: the smallest
    relative distance of a decision from its cutoff; ``shape_gap``)."""
    S = len(pos)
    for rnd in range(VR.MAX_ROUNDS):
        R = VR.radius(cell, S, rnd)
        q, sid = site_neighbours(cell, pos, c, R)
        faces = site_round(q, R)
        if faces is not None:
            break
    else:
        raise RuntimeError("the cell of the site does not close")
    d = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    js = sorted(faces)
    d_min, w_max = min(d[j] for j in js), max(faces[j] for j in js)
    chosen, nd, na, margin = [], [], [], np.inf
    for j in js:
        rd, ra = d[j] / d_min, faces[j] / w_max
        if rd <= distance_cutoff:                                     # the angle only matters for a face that passes the distance
            margin = min(margin, abs(ra - angle_cutoff) / angle_cutoff)
        if ra >= angle_cutoff:
            margin = min(margin, abs(rd - distance_cutoff) / distance_cutoff)
        if rd <= distance_cutoff and ra >= angle_cutoff:
            chosen.append(j); nd.append(rd); na.append(ra)
    n = len(chosen)
    symbol, best, all3, conf, gap = decide(n, q[chosen], max_csm)
    return {"rounds": rnd + 1, "final_radius": R, "n": n, "vertices": [int(sid[j]) for j in chosen], "norm_distance": np.array(nd),
            "norm_angle": np.array(na), "symbol": symbol, "csm_best": best, "csm_all": all3, "confidence": conf, "select_margin": margin,
            "shape_gap": gap, "nbr_count": len(q), "q": q[chosen]}


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def _grid(G):
    return np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)


def fcc():
    basis = np.array([(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)])
    return np.eye(3) * 8.0, (_grid(2)[:, None, :] + basis[None]).reshape(-1, 3) * 4.0


def bcc():
    g = _grid(3)
    return np.eye(3) * 9.0, np.concatenate([g, g + 0.5]) * 3.0


def sc():
    return np.eye(3) * 9.0, _grid(3) * 3.0


def fcc1_rounded():
    """The conventional FCC cell (a = 4, 4 atoms) with coordinates that went through + 0.3 - 0.3: the holes are collinear with
    opposite atoms only up to a rounding, and every neighbour is an image of one of four atoms."""
    basis = np.array([(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)]) * 4.0
    return np.eye(3) * 4.0, (basis + 0.3) - 0.3


def gaussian(cell_pos, sigma, seed):
    cell, pos = cell_pos
    return cell, pos + np.random.default_rng(seed).normal(0.0, sigma, pos.shape)


def cluster(seventh):
    """A unit octahedron about the site at the centre of a 12 A cubic cell, a 7th atom along (1, 1, 1) and 8 far atoms at
    (+-3, +-3, +-3) that close the cell."""
    o = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    far = np.array([[x, y, z] for x in (3.0, -3.0) for y in (3.0, -3.0) for z in (3.0, -3.0)])
    return np.eye(3) * 12.0, np.concatenate([o, seventh * np.ones((1, 3)) / np.sqrt(3.0), far]) + 6.0


def shell(S, seed):
    """S atoms at 3 A (+- 1%) from the site at the centre of a 30 A cell: every one of them coordinates it."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(S, 3))
    v *= (3.0 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, S)) / np.linalg.norm(v, axis=1))[:, None]
    return np.eye(3) * 30.0, v + 15.0


FCC_SITES = np.array([[2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [6.0, 2.0, 6.0], [3.0, 5.0, 7.0]])          # octahedral, tetrahedral, again
BCC_SITES = np.array([[1.5, 0.75, 0.0], [1.5, 1.5, 0.0], [4.5, 3.0, 3.75]])
SC_SITES = np.array([[1.5, 1.5, 1.5], [4.5, 7.5, 1.5]])
CENTRE12 = np.array([[6.0, 6.0, 6.0]])

FIXTURES = {
    "fcc": lambda: fcc() + (FCC_SITES,),
    "bcc": lambda: bcc() + (BCC_SITES,),
    "sc": lambda: sc() + (SC_SITES,),
    "fcc1_rounded": lambda: fcc1_rounded() + (np.array([[2.0, 2.0, 2.0], [2.0, 0.0, 0.0], [1.0, 1.0, 1.0], [3.0, 1.0, 3.0]]),),
    "fcc_jitter": lambda: gaussian(fcc(), 0.08, 11) + (FCC_SITES,),
    "bcc_jitter": lambda: gaussian(bcc(), 0.06, 12) + (BCC_SITES[[0, 2]],),      # not the L:2 site: its second shell is 1% off the cutoff
    "sc_jitter": lambda: gaussian(sc(), 0.06, 13) + (SC_SITES,),
    "cluster_1.2": lambda: cluster(1.2) + (CENTRE12,),
    "cluster_1.1": lambda: cluster(1.1) + (CENTRE12,),
    "small_triclinic": lambda: VR.fixture("small_triclinic") + (np.array([[0.5, 0.5, 0.5], [0.15, 0.7, 0.35]]) @ BR.SMALL_TRICLINIC,),
    "sc_void": lambda: VR.sc_void() + (np.array([[9.0, 9.0, 9.0], [9.0, 9.0, 7.0], [7.0, 7.0, 7.0]]),),
}
# what the issue states for the ideal lattices and the cluster: (n, symbol) per site
EXPECTED = {
    "fcc": [(6, "O:6"), (4, "T:4"), (6, "O:6"), (4, "T:4")],
    "fcc1_rounded": [(6, "O:6"), (6, "O:6"), (4, "T:4"), (4, "T:4")],
    "bcc": [(4, "T:4"), (2, "L:2"), (4, "T:4")],
    "sc": [(8, "C:8"), (8, "C:8")],
    "fcc_jitter": [(6, "O:6"), (4, "T:4"), (6, "O:6"), (4, "T:4")],
    "bcc_jitter": [(4, "T:4"), (4, "T:4")],
    "sc_jitter": [(8, "C:8"), (8, "C:8")],
    "cluster_1.2": [(6, "O:6")],
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    cell, pos, sites = FIXTURES[name]()
    return np.asarray(cell, dtype=np.float64), np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(sites, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def answer(name):
    """The restatement's answer for every site of a fixture, computed once and shared."""
    cell, pos, sites = fixture(name)
    return [site(cell, pos, c) for c in sites]
