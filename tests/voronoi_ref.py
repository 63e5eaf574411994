"""The contract of ``VoronoiSiteGenerator`` (sitator_amd/csrc/voronoi_plan.h) restated in numpy, brute force, with the same
``tau`` / ``mu`` rules, the same enumeration order and the same record rules, and an exact evaluation
(``fractions.Fraction`` on the float inputs) of a quadruple's circumcentre and of the shell distances, which
tests/test_voronoi_ref.py uses to show that every fixture is far from every threshold.

There is no golden from the true reference for this operator: the reference gets its nodes from the external Zeo++ ``network``
binary, which cannot be run here.  The yardsticks are qhull (``scipy.spatial.Voronoi`` over a 5 x 5 x 5 block of periodic images,
tests/make_voronoi_golden.py -> tests/golden/voronoi_known_answers.npz) for generic inputs and the lattices whose nodes are
known in closed form (sitator_amd/synth.py) for degenerate ones.

The restatement decides on plain float64 comparisons (it certifies nothing): it is only valid on inputs that are far from every
threshold, which ``margins`` measures."""
import functools
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

from sitator_amd import synth
from tests import barrier_ref as BR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "voronoi_known_answers.npz")

OK, GROW, UNCERTAIN, CAPACITY = 0, 1, 2, 3
NBR_CAP, REC_CAP, MEMBER_CAP, MAX_ROUNDS = 256, 128, 32, 12
R0_FACTOR, GROWTH = 2.125, 1.3
SHAPE_MIN = 1.0 / 131072.0
MU_FACTOR = 16.0
EPS = 2.0 ** -53
BOUND_A = (7.0 + 56.0 * EPS) * EPS
TAU = 1e-6

# The largest |header centre - exact centre| (both wrapped into the cell) and |header radius - exact radius| over the nodes of
# every generic fixture, measured by the host probe: 1.06e-13, on a sliver of sc3_jitter (tests/test_voronoi_plan.py prints the measurement and fails if a later
# one exceeds it).  CENTER_TOL has the margin hull_ref.QHULL_REL_TOL has, for the same reason: the device may round in another
# order (it does not: both compilers are told -ffp-contract=off, but nothing here relies on that).
CENTER_MEASURED = 1.07e-13
CENTER_TOL = 64 * CENTER_MEASURED

getcontext().prec = 60


def cell_inverse(cell):
    return np.ascontiguousarray(np.linalg.inv(np.asarray(cell, dtype=np.float64).T))    # as _lib.HipContext makes it


def radius(cell, S, rnd):
    R = R0_FACTOR * float(np.cbrt(abs(np.linalg.det(np.asarray(cell, dtype=np.float64))) / float(S)))
    for _ in range(rnd):
        R *= GROWTH
    return R


def wrap(cell, pts):
    cell = np.asarray(cell, dtype=np.float64)
    ci, cm = cell_inverse(cell), cell.T
    f = np.asarray(pts, dtype=np.float64) @ ci.T
    f -= np.floor(f)
    return f @ cm.T


def neighbours(cell, pos, i, R):
    """``(q [n, 3], sid [n], m [n, 3])``: every atom image within R of atom i (not itself), relative to it, in the order
    (squared distance, static index, m0, m1, m2) - the arithmetic of vp_relative."""
    cell = np.asarray(cell, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    ci = cell_inverse(cell)
    h = BR.heights(cell)
    g = (pos[i] - pos) @ ci.T                                         # [S, 3] crystal coordinates of p_i - p_s
    reach = np.ceil(R / h) + 1
    lo = np.floor(g.min(axis=0) - reach).astype(np.int64)
    hi = np.ceil(g.max(axis=0) + reach).astype(np.int64)
    m = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    mf = m.astype(np.float64)
    T = np.stack([(mf[:, 0] * cell[0, k] + mf[:, 1] * cell[1, k]) + mf[:, 2] * cell[2, k] for k in range(3)], axis=1)
    out_q, out_s, out_m, out_d = [], [], [], []
    for s in range(len(pos)):
        d = (pos[i] - pos[s])[None, :] - T
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 <= R * R
        if s == i:
            keep &= np.any(m != 0, axis=1)
        if keep.any():
            out_q.append(-d[keep]); out_m.append(m[keep]); out_d.append(d2[keep]); out_s.append(np.full(int(keep.sum()), s))
    if not out_q:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64)
    q, m, d2, s = np.concatenate(out_q), np.concatenate(out_m), np.concatenate(out_d), np.concatenate(out_s)
    order = np.lexsort((m[:, 2], m[:, 1], m[:, 0], s, d2))
    return q[order], s[order].astype(np.int64), m[order]


def det_permanent(a, b, c):
    """hp_det(a, b, c, 0) and its permanent, the header's operation order; arrays [..., 3]."""
    adx, ady, adz = a[..., 0], a[..., 1], a[..., 2]
    bdx, bdy, bdz = b[..., 0], b[..., 1], b[..., 2]
    cdx, cdy, cdz = c[..., 0], c[..., 1], c[..., 2]
    bdxcdy, cdxbdy = bdx * cdy, cdx * bdy
    cdxady, adxcdy = cdx * ady, adx * cdy
    adxbdy, bdxady = adx * bdy, bdx * ady
    det = adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy) + cdz * (adxbdy - bdxady)
    perm = (np.abs(bdxcdy) + np.abs(cdxbdy)) * np.abs(adz) + (np.abs(cdxady) + np.abs(adxcdy)) * np.abs(bdz) \
        + (np.abs(adxbdy) + np.abs(bdxady)) * np.abs(cdz)
    return det, perm


def shape_ok(a, b, c):
    det, perm = det_permanent(a, b, c)
    return (np.abs(det) > BOUND_A * perm) & (np.abs(det) >= SHAPE_MIN * perm), det, perm


def spheres(a, b, c):
    """``(valid, u, r, ratio)`` of vp_sphere for arrays [..., 3]."""
    valid, det, perm = shape_ok(a, b, c)
    wa = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    wb = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
    wc = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
    den = 2.0 * det
    u = np.zeros(a.shape)
    with np.errstate(all="ignore"):
        for x in range(3):
            y, z = (x + 1) % 3, (x + 2) % 3
            N = (wa * (b[..., y] * c[..., z] - b[..., z] * c[..., y]) + wb * (c[..., y] * a[..., z] - c[..., z] * a[..., y])) \
                + wc * (a[..., y] * b[..., z] - a[..., z] * b[..., y])
            u[..., x] = N / den
        r = np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
        ratio = np.abs(det) / perm
    return valid, u, r, ratio


def octants(q):
    mask = 0
    for v in q:
        if np.all(v != 0.0):
            mask |= 1 << int((v[0] < 0) + 2 * (v[1] < 0) + 4 * (v[2] < 0))
    return mask


def triples(n):
    """All a < b < c below n, lexicographic."""
    idx = np.arange(n)
    a, b = np.nonzero(idx[:, None] < idx[None, :])
    out = []
    for lo in range(0, len(a), 4096):                                 # in pieces: n = 200 has 1.3 million of them
        aa, bb = a[lo:lo + 4096], b[lo:lo + 4096]
        cc = idx[None, :].repeat(len(aa), axis=0)
        keep = cc > bb[:, None]
        out.append(np.stack([aa[:, None].repeat(n, axis=1)[keep], bb[:, None].repeat(n, axis=1)[keep], cc[keep]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


def atom_round(q, sid, self_sid, R, tau, margins=None):
    """One atom at one search radius: ``(status, records, n_far)``; a record is ``(u, r, member static indices with the atom
    first, (a, b, c))``, in enumeration order.  ``margins`` (a dict) collects how far the decisions were from their thresholds."""
    n = len(q)
    if n > NBR_CAP:
        return CAPACITY, [], 0
    tri = triples(n)
    records, n_far, capacity = [], 0, False
    PRE = 12
    for lo in range(0, len(tri), 200000):
        t = tri[lo:lo + 200000]
        valid, u, r, _ = spheres(q[t[:, 0]], q[t[:, 1]], q[t[:, 2]])
        keep = np.nonzero(valid)[0]
        # nearest neighbours first: most spheres hold one of them well inside and go no further
        worst = np.full(len(t), np.inf)
        for first, last in ((0, min(PRE, n)), (min(PRE, n), min(5 * PRE, n)), (min(5 * PRE, n), n)):
            if last <= first or not len(keep):
                continue
            cols = np.arange(first, last)
            gap = np.linalg.norm(q[None, first:last, :] - u[keep, None, :], axis=2) - r[keep, None]
            own = (t[keep, 0, None] == cols) | (t[keep, 1, None] == cols) | (t[keep, 2, None] == cols)
            worst[keep] = np.minimum(worst[keep], np.where(own, np.inf, gap).min(axis=1))
            keep = keep[worst[keep] > -100.0 * tau]
        if margins is not None and len(keep):                          # an inside / not inside answer within 100 tau of its threshold
            near = r[keep] <= 0.5 * R
            margins["inside_band"] = margins.get("inside_band", 0) + int(np.count_nonzero(near & (worst[keep] < -tau / 100.0)))
        keep = keep[worst[keep] >= -tau]
        far = ~(r[keep] <= 0.5 * R)
        n_far += int(np.count_nonzero(far))
        keep = keep[~far]
        if margins is not None and len(keep):
            margins["half_R"] = min(margins.get("half_R", np.inf), float((0.5 * R - r[keep]).min()))
        for k in keep:
            a, b, c = (int(v) for v in t[k])
            d = np.sqrt(((q - u[k]) ** 2).sum(axis=1))
            on = np.abs(d - r[k]) <= tau
            on[[a, b, c]] = True
            members = [int(j) for j in np.nonzero(on)[0]]
            if len(members) > MEMBER_CAP - 1:
                capacity = True
                continue
            if sid[on].min() < self_sid:
                continue
            first = None
            for x in range(len(members)):
                for y in range(x + 1, len(members)):
                    for z in range(y + 1, len(members)):
                        if first is None and shape_ok(q[members[x]], q[members[y]], q[members[z]])[0]:
                            first = (members[x], members[y], members[z])
                    if first is not None:
                        break
                if first is not None:
                    break
            if first != (a, b, c):
                continue
            records.append((u[k].copy(), float(r[k]), [int(self_sid)] + [int(sid[j]) for j in members], (a, b, c)))
    if len(records) > REC_CAP:
        capacity = True
    if capacity:
        return CAPACITY, [], n_far
    if octants(q) != 0xFF or n_far:
        return GROW, [], n_far
    return OK, records, n_far


def merge(cell, w, mu):
    """``(status, node of every record, first record of every node)`` of vp_merge, all pairs."""
    cell = np.asarray(cell, dtype=np.float64)
    n = len(w)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    ambiguous = False
    if n:
        ci = cell_inverse(cell)
        f = w @ ci.T
        f -= np.floor(f)
        for k in range(1, n):
            df = f[k] - f[:k]
            df -= np.rint(df)
            dist = np.linalg.norm(df @ cell, axis=1)
            ambiguous = ambiguous or bool(((dist > mu) & (dist <= 4.0 * mu)).any())
            for j in np.nonzero(dist <= mu)[0]:
                rk, rj = find(k), find(int(j))
                if rk < rj:
                    parent[rj] = rk
                elif rj < rk:
                    parent[rk] = rj
    node, first = [-1] * n, []
    for k in range(n):
        r = find(k)
        if r == k:
            node[k] = len(first)
            first.append(k)
        else:
            node[k] = node[r]
    return (UNCERTAIN if ambiguous else OK), np.array(node, dtype=np.int64), np.array(first, dtype=np.int64)


def nodes(cell, pos, tau=TAU, with_margins=False):
    """The whole operator: a dict of ``centers`` (wrapped), ``radii``, ``vertices`` (sorted unique static indices per node),
    ``status`` [S], ``nbr_count`` [S], ``rounds``, ``final_radius``, ``records`` and, per node, ``quad`` = (atom, q_a, q_b, q_c) of
    its first record (for the exact centre)."""
    cell = np.asarray(cell, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    S = len(pos)
    status = np.full(S, GROW, dtype=np.int32)
    nbr = np.zeros(S, dtype=np.int32)
    recs = [[] for _ in range(S)]
    active, rounds, R = list(range(S)), 0, 0.0
    margins = {} if with_margins else None
    while active:
        if rounds >= MAX_ROUNDS or not radius(cell, S, rounds) / BR.heights(cell).min() < 255.0:
            status[active] = CAPACITY
            break
        R = radius(cell, S, rounds)
        rounds += 1
        nxt = []
        for i in active:
            q, sid, _ = neighbours(cell, pos, i, R)
            nbr[i] = len(q)
            if margins is not None and len(q):
                margins["R_shell"] = min(margins.get("R_shell", np.inf), float(np.abs(np.linalg.norm(q, axis=1) - R).min()))
            st, rec, _ = atom_round(q, sid, i, R, tau, margins)
            status[i] = st
            if st == GROW:
                nxt.append(i)
            elif st == OK:
                recs[i] = [(i, q, rec_k) for rec_k in rec]
        active = nxt
    out = {"status": status, "nbr_count": nbr, "rounds": rounds, "final_radius": R, "margins": margins,
           "centers": np.zeros((0, 3)), "radii": np.zeros(0), "vertices": [], "quad": [], "records": 0, "merge_status": OK}
    if not np.all(status == OK):
        return out
    flat = [r for per in recs for r in per]
    out["records"] = len(flat)
    w = wrap(cell, np.array([pos[i] + rec[0] for i, _, rec in flat]).reshape(-1, 3))
    st, node, first = merge(cell, w, MU_FACTOR * tau)
    out["merge_status"] = st
    if st != OK:
        return out
    verts = [set() for _ in first]
    for k, (_, _, rec) in enumerate(flat):
        verts[node[k]].update(rec[2])
    out["vertices"] = [sorted(v) for v in verts]
    out["centers"] = w[first]
    out["radii"] = np.array([flat[k][2][1] for k in first])
    out["quad"] = [(flat[k][0], flat[k][1][list(flat[k][2][3])]) for k in first]
    out["all_quads"] = [(i, q[list(rec[3])], q, rec) for i, q, rec in flat]
    return out


# ---- exact evaluation -----------------------------------------------------------------------------------------------------------

def exact_center(qa, qb, qc):
    """The circumcentre of (0, qa, qb, qc), exactly, as three Fractions."""
    A = [[Fraction(float(v)) for v in row] for row in (qa, qb, qc)]
    w = [sum(v * v for v in row) for row in A]

    def det3(M):
        return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
                + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))
    D = det3(A)
    if D == 0:
        return None
    out = []
    for x in range(3):
        M = [[(w[k] / 2 if j == x else A[k][j]) for j in range(3)] for k in range(3)]
        out.append(det3(M) / D)
    return out


def _sqrt(fr):
    return (Decimal(fr.numerator) / Decimal(fr.denominator)).sqrt()


def exact_radius(u):
    return _sqrt(sum(v * v for v in u))


def exact_gaps(u, q):
    """d - r for every row of q against the exact sphere of centre u through the origin, as Decimals (60 digits)."""
    r = exact_radius(u)
    return [_sqrt(sum((Fraction(float(v)) - c) ** 2 for v, c in zip(row, u))) - r for row in q]


def exact_ratio(qa, qb, qc):
    """|det| / permanent of the quadruple, exactly (a float of the exact quotient)."""
    A = [[Fraction(float(v)) for v in row] for row in (qa, qb, qc)]
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = A
    det = az * (bx * cy - cx * by) + bz * (cx * ay - ax * cy) + cz * (ax * by - bx * ay)
    perm = (abs(bx * cy) + abs(cx * by)) * abs(az) + (abs(cx * ay) + abs(ax * cy)) * abs(bz) + (abs(ax * by) + abs(bx * ay)) * abs(cz)
    return float(abs(det) / perm)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def sc(G, a=4.0):
    g = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    return np.eye(3) * (a * G), (g + 0.25) * a


def bcc(G, a=4.2):
    g = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    return np.eye(3) * (a * G), np.concatenate([g + 0.1, g + 0.6]) * a


def fcc(G, a=5.0):
    g = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    basis = np.array([(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)])
    return np.eye(3) * (a * G), ((g[:, None, :] + basis[None] + 0.1).reshape(-1, 3)) * a


def jitter(cell_pos, amount, seed):
    cell, pos = cell_pos
    rng = np.random.default_rng(seed)
    return cell, pos + rng.uniform(-amount, amount, pos.shape)


def spread(cell, S, seed, outside=False):
    """S atoms in the cell, none closer to another (under the minimum image) than 0.72 of the mean spacing: random, but every
    Voronoi cell closes within three rounds of the search radius."""
    cell = np.asarray(cell, dtype=np.float64)
    rng = np.random.default_rng(seed)
    dmin = 0.72 * (abs(np.linalg.det(cell)) / S) ** (1.0 / 3.0)
    pts = []
    while len(pts) < S:
        p = rng.uniform(0.0, 1.0, 3) @ cell
        if all(np.linalg.norm(synth.mic_displacement(p - x, cell)) >= dmin for x in pts):
            pts.append(p)
    pos = np.array(pts)
    if outside:
        pos = pos + rng.integers(-3, 4, (S, 3)).astype(np.float64) @ cell
    return cell, pos


def sc_void():
    """SC 4^3 with a 2 x 2 x 2 block of atoms removed: the sphere of the void has 24 atoms on it and r = 1.658 a."""
    cell, pos = sc(4)
    g = np.rint(pos / 4.0 - 0.25).astype(int)
    keep = ~np.all((g >= 1) & (g <= 2), axis=1)
    return cell, pos[keep]


GENERIC = {                                                           # the golden has qhull's answer for these
    "bcc2_jitter": lambda: jitter(bcc(2), 0.2, 1),
    "fcc2_jitter": lambda: jitter(fcc(2), 0.2, 2),
    "sc3_jitter": lambda: jitter(sc(3), 0.15, 6),
    "spread63": lambda: spread(np.eye(3) * 14.0, 63, 63),
    "spread64": lambda: spread(np.eye(3) * 14.0, 64, 165),
    "spread65": lambda: spread(np.eye(3) * 14.0, 65, 65),
    "triclinic": lambda: spread(BR.TRICLINIC, 40, 7, outside=True),
    "small_triclinic": lambda: spread(BR.SMALL_TRICLINIC, 3, 8, outside=True),
}
IDEAL = {
    "sc1": lambda: sc(1),
    "bcc1": lambda: bcc(1),
    "sc2": lambda: sc(2),
    "bcc2": lambda: bcc(2),
    "fcc2": lambda: fcc(2),
    "sc_void": sc_void,
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    cell, pos = (GENERIC.get(name) or IDEAL[name])()
    return np.asarray(cell, dtype=np.float64), np.ascontiguousarray(pos, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def answer(name):
    """The restatement's answer for a fixture, computed once and shared."""
    cell, pos = fixture(name)
    return nodes(cell, pos, TAU, with_margins=True)


def golden():
    return np.load(GOLDEN)


def qhull_nodes(cell, pos, block=2):
    """Voronoi nodes from qhull over a (2 block + 1)^3 block of images: ``(centers wrapped, vertex sets)`` of the distinct
    vertices with their centre in the cell, each with the static indices of the points whose regions meet there."""
    from scipy.spatial import Voronoi
    cell = np.asarray(cell, dtype=np.float64)
    S = len(pos)
    rng = range(-block, block + 1)
    shifts = np.array([[i, j, k] for i in rng for j in rng for k in rng], dtype=np.float64)
    pts = (wrap(cell, pos)[None, :, :] + (shifts @ cell)[:, None, :]).reshape(-1, 3)
    vor = Voronoi(pts)
    owners = {}
    for point, region in enumerate(vor.point_region):
        for v in vor.regions[region]:
            if v >= 0:
                owners.setdefault(v, set()).add(point)
    found = {}
    ci = cell_inverse(cell)
    for v, points in owners.items():
        c = vor.vertices[v]
        f = ci @ c
        if not np.all((f >= 0.0) & (f < 1.0)):                       # one copy of every node: its centre in the home cell
            continue
        found[tuple(np.round(c, 6))] = (c, frozenset(int(p) % S for p in points))
    keys = sorted(found)
    return np.array([found[k][0] for k in keys]).reshape(-1, 3), [sorted(found[k][1]) for k in keys]


def exact_wrap(cell, c):
    """Three Fractions wrapped into the cell the way cp_wrap does it, exactly: floats."""
    cell = np.asarray(cell, dtype=np.float64)
    ci = [[Fraction(float(v)) for v in row] for row in cell_inverse(cell)]
    f = [sum(ci[a][k] * c[k] for k in range(3)) for a in range(3)]
    f = [v - (v.numerator // v.denominator) for v in f]
    return np.array([float(sum(Fraction(float(cell[j, k])) * f[j] for j in range(3))) for k in range(3)])


def exact_node(cell, pos, atom, quad):
    """``(wrapped centre, radius)`` of the sphere through atom ``atom`` and the three relative points ``quad``, exactly."""
    u = exact_center(*quad)
    c = [Fraction(float(pos[atom][k])) + u[k] for k in range(3)]
    return exact_wrap(cell, c), float(exact_radius(u))


def stored(name):
    """The restatement's answer for a fixture as tests/make_voronoi_golden.py stored it (tests/test_voronoi_ref.py recomputes
    every one of them): the GPU tests read this, the void fixture alone takes the restatement a minute."""
    g, k = golden(), "ref/" + name + "/"
    off = g[k + "offsets"]
    return {"centers": g[k + "centers"], "radii": g[k + "radii"], "exact_centers": g[k + "exact_centers"],
            "exact_radii": g[k + "exact_radii"], "vertices": [g[k + "indices"][off[j]:off[j + 1]].tolist() for j in range(len(off) - 1)],
            "status": g[k + "status"], "nbr_count": g[k + "nbr_count"], "rounds": int(g[k + "rounds"]),
            "final_radius": float(g[k + "final_radius"]), "records": int(g[k + "records"])}


def closed_form(name):
    """The node centres of an ideal lattice fixture in closed form (the interstitial positions sitator_amd/synth.py writes down),
    wrapped into the cell: SC cube centres; BCC tetrahedral sites; FCC tetrahedral then octahedral sites."""
    cell, _ = fixture(name)
    G = {"sc1": 1, "sc2": 2, "bcc1": 1, "bcc2": 2, "fcc2": 2}[name]
    g = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    a = cell[0, 0] / G
    if name.startswith("sc"):
        frac = g + 0.75
    elif name.startswith("bcc"):
        frac = (g[:, None, :] + synth._BCC_TET[None] + 0.1).reshape(-1, 3)
    else:
        frac = np.concatenate([(g[:, None, :] + synth._FCC_TET[None] + 0.1).reshape(-1, 3),
                               (g[:, None, :] + synth._FCC_OCT[None] + 0.1).reshape(-1, 3)])
    return wrap(cell, frac * a)
