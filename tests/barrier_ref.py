"""Shared by tests/test_barrier_ref.py, tests/test_barrier_plan.py (CPU), tests/test_gpu_barrier.py (GPU) and
tools/make_barrier_goldens.py: a plain numpy restatement of ``MergeSitesByBarrier`` with the truncated and shifted 12-6
potential of ``sitator_amd.calculators.LennardJones``, written from the formulas and not from the kernel; the designed cases;
and the goldens of the TRUE reference (tests/golden/barrier_known_answers.npz).

The potential.  ``d = (x - s) - T`` with ``T = (m0 cell[0] + m1 cell[1]) + m2 cell[2]``, ``d2 = (d0 d0 + d1 d1) + d2 d2``,
``s6 = (sigma^2 / d2)^3`` as ``(q q) q``, ``phi = (4 eps s6)(s6 - 1) - e0``, ``e0`` the same at ``d2 = rc rc``, counted where
``d2 <= rc rc``: numpy's IEEE operations in this order, so a single term is the same bits wherever it is evaluated.  The sum over
the terms is ``math.fsum`` (correctly rounded): the reference a reordered float64 sum is measured against.
"""
import itertools
import json
import math
import os

import numpy as np
from scipy.sparse.csgraph import connected_components

from tests import group_ref as GR
from tests import pathway_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "barrier_known_answers.npz")
CUBIC = np.eye(3) * 12.0
TRICLINIC = np.array([[12.0, 0.0, 0.0], [-2.0, 11.8, 0.0], [1.5, -1.0, 12.2]])
SMALL_TRICLINIC = np.array([[4.0, 0.0, 0.0], [0.8, 3.8, 0.0], [0.5, 0.6, 3.9]])
MARGIN = 1e-6                # of max |E| of a pair: how far every decision of a golden case stays from its tie


# ---- the potential -----------------------------------------------------------------------------------------------------------

def lj_parameters(numbers, epsilon, sigma):
    """(eps [S], sigma [S]) from scalars or ``{atomic number: value}`` dicts."""
    numbers = np.asarray(numbers, dtype=np.int64).reshape(-1)

    def per_atom(v):
        if isinstance(v, dict):
            return np.array([float(v[int(z)]) for z in numbers], dtype=np.float64)
        return np.full(len(numbers), float(v))
    return per_atom(epsilon), per_atom(sigma)


def lj(d2, sig2, eps4):
    with np.errstate(divide="ignore", over="ignore"):
        q = sig2 / d2
        s6 = (q * q) * q
        return (eps4 * s6) * (s6 - 1.0)


def atom_constants(eps, sigma, rc):
    """(eps4, sig2, e0) per atom."""
    eps, sigma = np.asarray(eps, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    eps4, sig2 = 4.0 * eps, sigma * sigma
    return eps4, sig2, lj(np.float64(rc) * np.float64(rc), sig2, eps4)


def phi(d2, sig2, eps4, e0):
    return lj(d2, sig2, eps4) - e0


def heights(cell):
    """The perpendicular heights of the cell along its three vectors."""
    cell = np.asarray(cell, dtype=np.float64)
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3])) for a in range(3)])


def plan_translations(cell, rc):
    """floor(rc / h_a) + 1: what covers every term once the difference of two points is brought into the cell."""
    return np.floor(rc / heights(cell)).astype(np.int64) + 1


def terms(cell, static_pos, eps, sigma, rc, x):
    """(phi, d2, atom, m) of every term within the cutoff of a mobile atom at ``x``: brute force over the triples
    ``rint(crystal(x - s)) + t``, ``|t_a| <= ceil(rc / h_a) + 2``."""
    cell = np.asarray(cell, dtype=np.float64)
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    x = np.asarray(x, dtype=np.float64)
    eps4, sig2, e0 = atom_constants(eps, sigma, rc)
    reach = np.ceil(rc / heights(cell)).astype(np.int64) + 2
    offs = np.array(list(itertools.product(*[range(-int(r), int(r) + 1) for r in reach])), dtype=np.float64)
    b = x[None, :] - static_pos                                                   # [S, 3]
    base = np.rint(b @ np.linalg.inv(cell))                                       # crystal coordinates of the difference
    m = base[:, None, :] + offs[None, :, :]                                       # [S, NT, 3]
    T = (m[..., 0:1] * cell[0] + m[..., 1:2] * cell[1]) + m[..., 2:3] * cell[2]
    d = b[:, None, :] - T
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    atom, which = np.nonzero(d2 <= np.float64(rc) * np.float64(rc))
    dd = d2[atom, which]
    return phi(dd, sig2[atom], eps4[atom], e0[atom]), dd, atom, m[atom, which].astype(np.int64)


def mobile_energy(cell, static_pos, eps, sigma, rc, x):
    """(E(x), sum |phi|, number of terms)."""
    p = terms(cell, static_pos, eps, sigma, rc, x)[0]
    if np.isinf(p).any():
        return np.inf, np.inf, len(p)
    return math.fsum(p), math.fsum(np.abs(p)), len(p)


def path_energies(cell, static_pos, eps, sigma, rc, points):
    """(E, sum |phi|, terms), each shaped like ``points[..., 0]``."""
    points = np.asarray(points, dtype=np.float64)
    flat = points.reshape(-1, 3)
    out = np.array([mobile_energy(cell, static_pos, eps, sigma, rc, x) for x in flat]).reshape(points.shape[:-1] + (3,))
    return out[..., 0], out[..., 1], out[..., 2].astype(np.int64)


def lattice_energy(cell, static_pos, eps, sigma, rc):
    """A constant in the spirit of the lattice's own energy: half the sum, over the atoms, of the energy of a probe at the
    atom's place among all the others and its own images."""
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    total = []
    for s in range(len(static_pos)):
        p, dd, _, _ = terms(cell, static_pos, eps, sigma, rc, static_pos[s])
        total.append(math.fsum(p[dd > 0.0]))
    return 0.5 * math.fsum(total)


# ---- the operator --------------------------------------------------------------------------------------------------------------

def pairwise_distances(cell, pts):
    """PBCCalculator.pairwise_distances (util/PBCCalculator.pyx:43-103): shift-and-wrap."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cen = GR.centroid(cell)
    n = len(pts)
    out = np.zeros((n, n))
    for i in range(n - 1):
        buf = pts[i + 1:] + (cen - pts[i])
        buf = -GR.wrap_points(cell, buf)
        buf += cen
        buf *= buf
        out[i, i + 1:] = np.sqrt(np.sum(buf, axis=1))
        out[i + 1:, i] = out[i, i + 1:]
    return out


def candidate_pairs(cell, centers, n_ij, maximum_pairwise_distance, minimum_jumps_mergable):
    """(mergable [K, K] before any barrier, pairs [P, 2] with i < j in the order of itertools.combinations)."""
    mergable = pairwise_distances(cell, centers) <= maximum_pairwise_distance
    mergable &= np.asarray(n_ij) >= minimum_jumps_mergable
    K = len(mergable)
    pairs = [p for p in itertools.combinations(range(K), r=2) if mergable[p] or mergable[p[1], p[0]]]
    return mergable, np.array(pairs, dtype=np.int64).reshape(-1, 2)


def driven_points(cell, centers, pairs, n):
    """(points [P, n, 3], codes [P]): vector * coeff + pos[i], vector to the min_image of pos[j]."""
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    coeffs = np.linspace(0, 1, n)
    if not len(pairs):
        return np.zeros((0, n, 3)), np.zeros(0, dtype=np.int64)
    moved, codes = PR.min_image(cell, centers[pairs[:, 0]], centers[pairs[:, 1]])
    vector = moved - centers[pairs[:, 0]]
    return (vector[:, None, :] * coeffs[None, :, None]) + centers[pairs[:, 0]][:, None, :], codes


def verdict(energies, threshold):
    """(interior, forward <= threshold, backward <= threshold) of one row of image energies."""
    energies = np.asarray(energies, dtype=np.float64)
    k = int(np.argmax(energies))
    with np.errstate(invalid="ignore"):
        forward, backward = energies[k] - energies[0], energies[k] - energies[-1]
        return k != 0 and k != len(energies) - 1, bool(forward <= threshold), bool(backward <= threshold)


def margins(energies, threshold):
    """(|barrier - threshold| of the nearer barrier, |max interior - max end|), both over max |E| of the row."""
    e = np.asarray(energies, dtype=np.float64)
    scale = np.max(np.abs(e))
    k = int(np.argmax(e))
    ends = max(e[0], e[-1])
    interior = np.max(e[1:-1])
    gap = abs(interior - ends) / scale
    if k in (0, len(e) - 1):
        return np.inf, gap
    return min(abs((e[k] - e[0]) - threshold), abs((e[k] - e[-1]) - threshold)) / scale, gap


def case_arrays(case):
    """(static_pos, eps, sigma, rc) of the coordinating atoms of a case."""
    mask = case["static_mask"] if case["coordinating_mask"] is None else case["coordinating_mask"]
    eps, sigma = lj_parameters(case["numbers"][mask], case["lj"]["epsilon"], case["lj"]["sigma"])
    return case["positions"][mask], eps, sigma, float(case["lj"]["rc"])


def sites_to_merge(case):
    """What ``_get_sites_to_merge`` computes: a dict of pairs, codes, energies [P, n] (mobile atom only), abs_sums, n_terms,
    mergable [K, K] and groups."""
    kw = case["kw"]
    n = kw.get("n_driven_images", 20)
    static_pos, eps, sigma, rc = case_arrays(case)
    mergable, pairs = candidate_pairs(case["cell"], case["centers"], case["n_ij"], kw.get("maximum_pairwise_distance", 2),
                                      kw.get("minimum_jumps_mergable", 1))
    points, codes = driven_points(case["cell"], case["centers"], pairs, n)
    energies, abs_sums, n_terms = path_energies(case["cell"], static_pos, eps, sigma, rc, points)
    for (i, j), row in zip(pairs, energies):
        interior, forward, backward = verdict(row, kw["barrier_threshold"])
        if interior:
            mergable[i, j], mergable[j, i] = forward, backward
    n_groups, labels = connected_components(mergable, directed=True, connection="strong")
    return {"pairs": pairs, "codes": codes, "points": points, "energies": energies, "abs_sums": abs_sums, "n_terms": n_terms,
            "mergable": mergable, "groups": [np.where(labels == g)[0] for g in range(n_groups)]}


def run_case(case):
    """``sites_to_merge`` and then ``MergeSites.run`` (network/merging.py:44-133): adds error (class name or ""), traj,
    centers and site_types of the merged trajectory."""
    out = sites_to_merge(case)
    kw, groups = case["kw"], out["groups"]
    out.update(error="", traj=None, centers=None, site_types=None)
    n_mobile = int(np.count_nonzero(case["mobile_mask"]))
    if len(groups) < n_mobile:
        out["error"] = "InsufficientSitesError"
        return out
    limit = kw.get("maximum_merge_distance", 2)
    table = np.full(len(case["centers"]), -1, dtype=np.int64)
    centers = np.empty((len(groups), 3))
    for new, g in enumerate(groups):
        table[g] = new
        pts = case["centers"][g]
        if limit is not None and len(g) > 1:
            d = pairwise_distances(case["cell"], pts)[0, 1:]
            if not np.all(d <= limit):
                out["error"] = "MergedSitesTooDistantError"
                return out
        centers[new] = GR.average(case["cell"], pts)
    traj = case["traj"]
    out["traj"] = np.where(traj == -1, -1, table[np.where(traj == -1, 0, traj)])
    out["centers"] = centers
    if kw.get("check_types", False):
        out["site_types"] = np.array([case["site_types"][g[0]] for g in groups], dtype=np.int64)
    return out


# ---- the designed cases ----------------------------------------------------------------------------------------------------

def _case(cell, static_pos, centers, n_ij, threshold, numbers=None, n_mobile=1, lj_kw=None, coordinating=None, site_types=None,
          traj=None, **kw):
    """A structure of the static atoms followed by ``n_mobile`` mobile ones (placed on the first centres)."""
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    S, K = len(static_pos), len(centers)
    positions = np.concatenate([static_pos, centers[np.arange(n_mobile) % K]])
    static_mask = np.arange(S + n_mobile) < S
    numbers = np.concatenate([np.full(S, 8) if numbers is None else np.asarray(numbers), np.full(n_mobile, 3)]).astype(np.int64)
    if traj is None:                                             # every ion walks over all sites; one unknown entry
        traj = (np.arange(2 * K)[:, None] + np.arange(n_mobile)[None, :]) % K
        traj[1, 0] = -1
    coordinating_mask = None
    if coordinating is not None:
        coordinating_mask = np.zeros(S + n_mobile, dtype=bool)
        coordinating_mask[np.asarray(coordinating)] = True
    lj_kw = dict(lj_kw or {})
    sigma = lj_kw.setdefault("sigma", 1.0)
    lj_kw.setdefault("epsilon", 1.0)
    lj_kw.setdefault("rc", 3.0 * (max(sigma.values()) if isinstance(sigma, dict) else sigma))
    kw = dict(kw, barrier_threshold=threshold)
    kw.setdefault("check_types", False)
    return {"cell": np.asarray(cell, dtype=np.float64), "positions": positions, "numbers": numbers, "static_mask": static_mask,
            "mobile_mask": ~static_mask, "centers": centers, "n_ij": np.asarray(n_ij, dtype=np.float64),
            "site_types": None if site_types is None else np.asarray(site_types, dtype=np.int64), "traj": traj.astype(np.int64),
            "coordinating_mask": coordinating_mask, "lj": lj_kw, "kw": kw}


def _both_ways(K, edges, jumps=2.0):
    n_ij = np.zeros((K, K))
    for a, b in edges:
        n_ij[a, b] = n_ij[b, a] = jumps
    return n_ij


A, B = np.array([3.0, 6.0, 6.0]), np.array([4.5, 6.0, 6.0])
MID = 0.5 * (A + B)
UP, DOWN = np.array([0.0, 1.0, 0.0]), np.array([0.0, -1.0, 0.0])


def golden_case_inputs():
    """name -> case.  One static atom beside the midpoint of two sites makes a double well whose barrier its distance sets;
    the kinds below are the ones tools/make_barrier_goldens.py asserts it covers."""
    cases = {}
    pair = _both_ways(2, [(0, 1)])
    # a double well with a low barrier (0.77 eps), one with a high barrier (7.6 eps)
    cases["low_barrier"] = _case(CUBIC, [MID + 1.0 * UP], [A, B], pair, 1.0)
    cases["high_barrier"] = _case(CUBIC, [MID + 0.9 * UP], [A, B], pair, 1.0)
    # the same double well across the cell boundary (min_image code 211) and in a triclinic cell
    shift = np.array([8.0, 0.0, 0.0])
    cases["low_barrier_across"] = _case(CUBIC, [MID + shift + 1.0 * UP], [A + shift, B + shift - CUBIC[0]], pair, 1.0)
    cases["high_barrier_triclinic"] = _case(TRICLINIC, [MID + 0.9 * UP, MID + 3.0 * DOWN], [A, B], pair, 1.0)
    # one basin: an atom behind A on the axis, the energy falls all the way to B; the entries stay as n_ij left them
    behind = A - np.array([1.2, 0.0, 0.0])
    cases["same_basin"] = _case(CUBIC, [behind], [A, B], pair, 0.01)
    one_way = np.zeros((2, 2))
    one_way[0, 1] = 3.0
    cases["same_basin_one_way"] = _case(CUBIC, [behind], [A, B], one_way, 0.01)
    # a deeper well at B: the barrier passes from A only
    cases["forward_only"] = _case(CUBIC, [MID + 1.0 * UP, B + 1.12 * DOWN], [A, B], pair, 0.8)
    # three sites 0.875 apart (their coordinates sum exactly in any order), the outer two never exchanged a jump: merged
    # through strong connectivity
    step = np.array([0.875, 0.0, 0.0])
    chain = [A, A + step, A + 2 * step]
    posts = [A + 0.5 * step + 1.0 * UP, A + 1.5 * step + 1.0 * DOWN]
    cases["chain_of_three"] = _case(CUBIC, posts, chain, _both_ways(3, [(0, 1), (1, 2)]), 1.5)
    # excluded before any energy: too few jumps, too far apart (no candidate pair at all)
    cases["too_few_jumps"] = _case(CUBIC, [MID + 1.0 * UP], [A, B], _both_ways(2, [(0, 1)], jumps=1.0), 1.0, minimum_jumps_mergable=2)
    far = A + np.array([2.5, 0.0, 0.0])
    cases["too_far_apart"] = _case(CUBIC, [0.5 * (A + far) + 1.3 * UP], [A, far], pair, 5.0)
    # the chain at 1.5: the outer sites end 3.0 apart in one group
    wide = np.array([1.5, 0.0, 0.0])
    cases["too_distant"] = _case(CUBIC, [A + 0.5 * wide + 1.0 * UP, A + 1.5 * wide + 1.0 * DOWN], [A, A + wide, A + 2 * wide],
                                 _both_ways(3, [(0, 1), (1, 2)]), 2.0)
    # two ions, two sites that merge
    cases["insufficient_sites"] = _case(CUBIC, [MID + 1.0 * UP], [A, B], pair, 1.0, n_mobile=2)
    # a second atom would close the path; the coordinating mask leaves it out
    cases["narrow_mask"] = _case(CUBIC, [MID + 1.0 * UP, MID + 0.9 * DOWN], [A, B], pair, 1.0, coordinating=[0])
    cases["full_mask"] = _case(CUBIC, [MID + 1.0 * UP, MID + 0.9 * DOWN], [A, B], pair, 1.0)
    # two species with their own epsilon and sigma, two site types; the third site is of the other type and on its own
    lone = np.array([9.0, 2.0, 3.0])
    cases["two_types"] = _case(CUBIC, [MID + 0.95 * UP, MID + 1.4 * DOWN, lone + 1.3 * UP], [A, B, lone], _both_ways(3, [(0, 1)]), 3.5,
                               numbers=[8, 16, 8], lj_kw={"epsilon": {8: 1.0, 16: 0.4}, "sigma": {8: 1.0, 16: 1.3}, "rc": 3.5},
                               site_types=[0, 0, 1], check_types=True, n_driven_images=9)
    # a cell shorter than the cutoff: a one-atom lattice, two sites on either side of a face of the cell, given inside it
    hollow = 0.8 * SMALL_TRICLINIC[0] + 0.2 * SMALL_TRICLINIC[1] + 0.3 * SMALL_TRICLINIC[2]
    other = 0.25 * SMALL_TRICLINIC[0] + 0.2 * SMALL_TRICLINIC[1] + 0.3 * SMALL_TRICLINIC[2]
    cases["small_cell_low"] = _case(SMALL_TRICLINIC, [np.zeros(3)], [hollow, other], pair, 40.0, lj_kw={"sigma": 1.6}, n_driven_images=7,
                                    maximum_pairwise_distance=2.5, maximum_merge_distance=2.5)
    cases["small_cell_high"] = _case(SMALL_TRICLINIC, [np.zeros(3)], [hollow, other], pair, 0.5, lj_kw={"sigma": 1.6}, n_driven_images=7,
                                     maximum_pairwise_distance=2.5, maximum_merge_distance=2.5)
    return cases


# what a case of each required kind looks like in the recorded results: name of the kind -> predicate on (case, result)
def coverage(case, res):
    kinds = set()
    K = len(case["centers"])
    merged = not res["error"] and len(res["groups"]) < K
    interior = [verdict(row, case["kw"]["barrier_threshold"]) for row in res["energies"]]
    if merged and any(v == (True, True, True) for v in interior) and K == 2:
        kinds.add("low barrier merges")
    if not merged and any(v == (True, False, False) for v in interior):
        kinds.add("high barrier does not merge")
    if any(not v[0] for v in interior):
        kinds.add("maximum at an end")
    if any(v[0] and v[1] != v[2] for v in interior) and not merged:
        kinds.add("forward only")
    if merged and K == 3 and len(res["groups"]) == 1 and len(res["pairs"]) == 2:
        kinds.add("chain of three")
    if case["kw"].get("minimum_jumps_mergable", 1) > 1 and len(res["pairs"]) == 0:
        kinds.add("excluded by jumps")
    if len(res["pairs"]) == 0 and (case["n_ij"] >= case["kw"].get("minimum_jumps_mergable", 1)).any():
        kinds.add("excluded by distance")
    if res["error"] == "MergedSitesTooDistantError":
        kinds.add("too distant")
    if res["error"] == "InsufficientSitesError":
        kinds.add("insufficient sites")
    if case["coordinating_mask"] is not None and (case["coordinating_mask"] != case["static_mask"]).any():
        kinds.add("narrow coordinating mask")
    if case["kw"].get("check_types") and len(set(case["site_types"].tolist())) == 2:
        kinds.add("two types")
    if (res["codes"] != 111).any():
        kinds.add("path across the boundary")
    if (np.asarray(case["lj"]["rc"]) > heights(case["cell"])).any():
        kinds.add("cell shorter than the cutoff")
    return kinds


KINDS = ["low barrier merges", "high barrier does not merge", "maximum at an end", "forward only", "chain of three",
         "excluded by jumps", "excluded by distance", "too distant", "insufficient sites", "narrow coordinating mask", "two types",
         "path across the boundary", "cell shorter than the cutoff"]


# ---- the goldens -------------------------------------------------------------------------------------------------------------

INPUT_KEYS = ["cell", "positions", "numbers", "static_mask", "mobile_mask", "centers", "n_ij", "traj"]


def case_to_blob(name, case):
    blob = {"%s/%s" % (name, k): case[k] for k in INPUT_KEYS}
    blob[name + "/site_types"] = np.zeros(0, dtype=np.int64) if case["site_types"] is None else case["site_types"]
    blob[name + "/coordinating_mask"] = np.zeros(0, dtype=bool) if case["coordinating_mask"] is None else case["coordinating_mask"]
    lj_kw = dict(case["lj"])
    for k in ("epsilon", "sigma"):
        if isinstance(lj_kw[k], dict):
            lj_kw[k] = {str(z): v for z, v in lj_kw[k].items()}
    blob[name + "/lj"] = json.dumps(lj_kw)
    blob[name + "/kw"] = json.dumps(case["kw"])
    return blob


class BarrierGoldens(object):
    def __init__(self):
        self.z = np.load(GOLDEN, allow_pickle=False)
        self.names = [str(n) for n in self.z["names"]]

    def case(self, name):
        z = self.z
        case = {k: z["%s/%s" % (name, k)] for k in INPUT_KEYS}
        types, mask = z[name + "/site_types"], z[name + "/coordinating_mask"]
        case["site_types"] = types if len(types) else None
        case["coordinating_mask"] = mask if len(mask) else None
        lj_kw = json.loads(str(z[name + "/lj"]))
        for k in ("epsilon", "sigma"):
            if isinstance(lj_kw[k], dict):
                lj_kw[k] = {int(zn): v for zn, v in lj_kw[k].items()}
        case["lj"] = lj_kw
        case["kw"] = json.loads(str(z[name + "/kw"]))
        return case

    def expected(self, name):
        pre = name + "/out_"
        out = {k[len(pre):]: self.z[k] for k in self.z.files if k.startswith(pre)}
        out["error"] = str(out["error"])
        out["groups"] = [out["group_members"][out["group_offsets"][g]:out["group_offsets"][g + 1]]
                         for g in range(len(out["group_offsets"]) - 1)]
        return out
