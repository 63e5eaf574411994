"""Shared by tests/test_pathway_ref.py, tests/test_pathway_graph.py (CPU), tests/test_gpu_pathways.py (GPU) and
tools/make_pathway_goldens.py: a numpy / scipy restatement of ``DiffusionPathwayAnalysis`` written for this project (dense
arrays, scipy's ``connected_components`` on the explicit supercell matrix), the designed and random inputs, and the goldens of
the TRUE reference (tests/golden/pathway_known_answers.npz).  The image decision uses ``clamp_ref.image_distances``: every
sum left to right, numpy's IEEE operations, the first minimum by ``argmin``."""
import itertools
import json
import numbers
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import clamp_ref as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pathway_known_answers.npz")
CUBIC = np.eye(3) * 10.0
TRICLINIC = np.array([[12.0, 0.0, 0.0], [-2.0, 11.8, 0.0], [1.5, -1.0, 12.2]])
IMAGES = np.array(list(itertools.product(range(-1, 2), repeat=3)))
HOME = 13
NO_PATHWAY = -1


# ---- the restatement --------------------------------------------------------------------------------------------------------

def connectivity(n_ij, threshold):
    n_ij = np.asarray(n_ij)
    if isinstance(threshold, numbers.Integral):
        return n_ij >= threshold
    if isinstance(threshold, numbers.Real):
        off = ~np.eye(len(n_ij), dtype=bool)
        return n_ij >= threshold * np.sum(n_ij[off])
    raise TypeError("threshold %r" % (threshold,))


def pair_codes(cell, centers, conn):
    """int32 [K, K]: 100 i + 10 j + k of the image of centers[to] nearest centers[from] for connected pairs, 0 elsewhere."""
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(conn.shape, dtype=np.int32)
    src, dst = np.nonzero(conn)
    if len(src):
        m = np.argmin(CR.image_distances(cell, centers[src], centers[dst]), axis=-1)
        out[src, dst] = 100 * (m // 9) + 10 * (m // 3 % 3) + m % 3
    return out


def min_image(cell, ref, pt):
    """(moved points, codes) for pairs ``ref[n, 3]``, ``pt[n, 3]``."""
    ref, pt = np.asarray(ref, dtype=np.float64).reshape(-1, 3), np.asarray(pt, dtype=np.float64).reshape(-1, 3)
    m = np.argmin(CR.image_distances(cell, ref, pt), axis=-1)
    return pt + CR.images(cell)[m], 100 * (m // 9) + 10 * (m // 3 % 3) + m % 3


def supercell_edges(conn, codes):
    """(u, v, dropped): the node pairs of the 27 K node graph, and how many (edge, image) pairs left the supercell."""
    K = len(conn)
    src, dst = np.nonzero(conn)
    shift = np.stack([codes[src, dst] // 100 - 1, codes[src, dst] // 10 % 10 - 1, codes[src, dst] % 10 - 1], axis=1)
    us, vs, dropped = [], [], 0
    for s, image in enumerate(IMAGES):
        target = image[None, :] + shift
        keep = np.all(np.abs(target) <= 1, axis=1)
        dropped += int(np.count_nonzero(~keep))
        t = 9 * (target[keep, 0] + 1) + 3 * (target[keep, 1] + 1) + (target[keep, 2] + 1)
        us.append(s * K + src[keep])
        vs.append(t * K + dst[keep])
    return np.concatenate(us), np.concatenate(vs), dropped


def component_labels(n_nodes, u, v):
    graph = coo_matrix((np.ones(len(u), dtype=bool), (u, v)), shape=(n_nodes, n_nodes))
    return connected_components(graph, directed=False)[1].astype(np.int64)


def ranked(root):
    """Component numbers in the order of each component's lowest node, from per-node representatives."""
    return np.unique(np.asarray(root), return_inverse=True)[1].reshape(-1).astype(np.int64)


def pathways_of(labels, K):
    """(site_pathway [K], directions: list of sets, candidates): dense masks, one component after the other; candidates =
    the components that touch the reference's "home" nodes and hold a site twice (more of them than pathways: some were
    merged).  Those nodes are 13 ... 13 + K - 1, as the reference marks them (it does not multiply the home image's index
    by K), not the K nodes of image 13."""
    grid = np.asarray(labels).reshape(27, K)
    masks, dirs, stamps = [], [], []
    stamp_of_site = np.zeros(K, dtype=np.int64)
    next_stamp, candidates = 1, 0
    for comp in range(int(grid.max()) + 1 if grid.size else 0):
        member = grid == comp
        if not member.reshape(-1)[HOME:HOME + K].any():
            continue
        times = member.sum(axis=0)
        if times.max() < 2:
            continue
        candidates += 1
        found = set()
        for site in np.flatnonzero(times >= 2):
            a, b = np.flatnonzero(member[:, site])[:2]
            found.add(tuple(IMAGES[a] != IMAGES[b]))
        mask = times > 0
        absorbed = [n for n, other in enumerate(masks) if (other & mask).any()]
        for n in absorbed:
            mask = mask | masks[n]
            found |= dirs[n]
        for n in reversed(absorbed):
            del masks[n], dirs[n], stamps[n]
        masks.append(mask)
        dirs.append(found)
        stamps.append(next_stamp)
        stamp_of_site[mask] = next_stamp
        next_stamp += 1
    site_pathway = np.full(K, NO_PATHWAY, dtype=np.int64)
    for number, stamp in enumerate(stamps):
        site_pathway[stamp_of_site == stamp] = number
    return site_pathway, dirs, candidates


def edge_matrix(site_pathway):
    same = site_pathway[:, None] == site_pathway[None, :]
    return np.where(same, site_pathway[:, None], NO_PATHWAY)


def directions_arrays(dirs):
    """A list of sets of triples as (uint8 [n, 3] - every set sorted -, int64 offsets [len + 1])."""
    rows, offsets = [], [0]
    for d in dirs:
        rows.extend(sorted(tuple(int(bool(x)) for x in t) for t in d))
        offsets.append(len(rows))
    return np.array(rows, dtype=np.uint8).reshape(-1, 3), np.array(offsets, dtype=np.int64)


def analyse(cell, centers, n_ij, connectivity_threshold=1, true_periodic_pathways=True, minimum_n_sites=0):
    """Everything a golden case stores, by the restatement."""
    K = len(centers)
    conn = connectivity(n_ij, connectivity_threshold)
    codes = pair_codes(cell, centers, conn)
    out = {"conn": conn, "codes": codes, "dropped": 0, "candidates": 0}
    if true_periodic_pathways:
        u, v, out["dropped"] = supercell_edges(conn, codes)
        labels = component_labels(27 * K, u, v)
        site, dirs, out["candidates"] = pathways_of(labels, K)
    else:
        u, v = np.nonzero(conn)
        labels = component_labels(K, u, v)
        sizes = np.bincount(labels)
        number = np.where(sizes >= minimum_n_sites, np.cumsum(sizes >= minimum_n_sites) - 1, NO_PATHWAY)
        site, dirs = number[labels], []
    out["labels"], out["site"], out["edge"] = labels, site, edge_matrix(site)
    out["count"] = int(site.max()) + 1 if K else 0
    out["dir_rows"], out["dir_offsets"] = directions_arrays(dirs)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _network(points, edges, both_ways=True, jumps=2.0):
    centers = np.array(points, dtype=np.float64)
    n_ij = np.zeros((len(centers), len(centers)))
    for a, b in edges:
        n_ij[a, b] = jumps
        if both_ways:
            n_ij[b, a] = jumps
    return centers, n_ij


def designed_cases():
    """name -> (cell, centers, n_ij, constructor keywords); all in the 10 A cubic cell."""
    out = {}
    chain_x = [(1.5, 5, 5), (5, 5, 5), (8.5, 5, 5)]
    ring = [(0, 1), (1, 2), (2, 0)]
    out["chain_x"] = _network(chain_x, ring)
    out["two_chains"] = _network([(1.5, 2, 2), (5, 2, 2), (8.5, 2, 2), (7, 1.5, 7), (7, 5, 7), (7, 8.5, 7)],
                                 ring + [(3, 4), (4, 5), (5, 3)])
    out["ring_and_chain"] = _network([(4, 4, 5), (6, 4, 5), (6, 6, 5), (4, 6, 5), (1.5, 1, 1), (5, 1, 1), (8.5, 1, 1)],
                                     [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 4)])
    out["half_cell"] = _network([(2.5, 5, 5), (7.5, 5, 5)], [(0, 1)])
    out["diagonal_xy"] = _network([(1.5, 1.5, 5), (5, 5, 5), (8.5, 8.5, 5)], ring)
    out["open_crossing"] = _network([(6, 5, 5), (8.5, 5, 5), (1.5, 5, 5), (4, 5, 5)], [(0, 1), (1, 2), (2, 3)])
    out["single_site"] = (np.array([[3.0, 4.0, 5.0]]), np.array([[2.0]]))
    out["no_edges"] = (np.array([(1.0, 1, 1), (4, 4, 4), (7, 7, 7), (2, 8, 5)]), np.zeros((4, 4)))
    out["one_way"] = _network(chain_x, ring, both_ways=False)
    # a chain around x and a site joined to it only across the y boundary: two components of the supercell touch the home
    # image, both reach an image of their own sites, and they share sites - the merge branch
    out["branch_across_y"] = _network([(1.5, 1.5, 5), (5, 1.5, 5), (8.5, 1.5, 5), (5, 8.5, 5)], ring + [(3, 1)])
    return {k: (CUBIC, v[0], v[1], {}) for k, v in out.items()}


def random_network(cell, K, seed, mean_degree=4.0, keep=0.75):
    """A random geometric graph: uniform centres, a directed edge i -> j with probability ``keep`` where the periodic
    distance is below the radius that gives ``mean_degree`` neighbours on average; 1 to 6 jumps on an edge."""
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=np.float64)
    centers = rng.uniform(size=(K, 3)) @ cell
    radius = (3.0 * mean_degree * abs(np.linalg.det(cell)) / (4.0 * np.pi * K)) ** (1.0 / 3.0)
    delta = centers[None, :, :] - centers[:, None, :]
    dist = np.min(np.linalg.norm(delta[:, :, None, :] + (IMAGES @ cell)[None, None, :, :], axis=-1), axis=-1)
    near = (dist < radius) & ~np.eye(K, dtype=bool) & (rng.random((K, K)) < keep)
    n_ij = np.where(near, rng.integers(1, 7, size=(K, K)), 0).astype(np.float64)
    return centers, n_ij


def snake(n=257, seed=3):
    """One closed path of ``n`` sites that goes once around x on a circle in y, z, neighbours joined both ways, the site
    indices permuted: the component of the supercell is one chain of 3 n nodes with its low indices scattered along it."""
    t = np.arange(n) / float(n)
    pts = np.stack([10.0 * t, 5.0 + 3.0 * np.sin(2 * np.pi * t), 5.0 + 3.0 * np.cos(2 * np.pi * t)], axis=1)
    perm = np.random.default_rng(seed).permutation(n)
    centers = np.empty_like(pts)
    centers[perm] = pts
    n_ij = np.zeros((n, n))
    for i in range(n):
        a, b = perm[i], perm[(i + 1) % n]
        n_ij[a, b] = n_ij[b, a] = 1.0
    return CUBIC, centers, n_ij


def golden_case_inputs():
    """Every golden case, in order: name -> (cell, centers, n_ij, keywords)."""
    cases = dict(designed_cases())
    for seed in (1, 2, 3):
        c, n = random_network(TRICLINIC, 60, seed)
        cases["tri60_s%d" % seed] = (TRICLINIC, c, n, {})
    c, n = random_network(TRICLINIC, 60, 1)
    cases["tri60_s1_int3"] = (TRICLINIC, c, n, {"connectivity_threshold": 3})
    cases["tri60_s1_frac"] = (TRICLINIC, c, n, {"connectivity_threshold": 0.008})
    cases["tri60_s1_plain_min0"] = (TRICLINIC, c, n, {"true_periodic_pathways": False})
    cases["tri60_s1_plain_min2"] = (TRICLINIC, c, n, {"true_periodic_pathways": False, "minimum_n_sites": 2})
    c, n = random_network(TRICLINIC, 65, 4)
    cases["tri65_s4"] = (TRICLINIC, c, n, {})
    c, n = random_network(TRICLINIC, 300, 5)
    cases["tri300_s5"] = (TRICLINIC, c, n, {"connectivity_threshold": 2})
    return cases


# ---- the goldens ------------------------------------------------------------------------------------------------------------

class PathwayGoldens(object):
    def __init__(self):
        self.z = np.load(GOLDEN, allow_pickle=False)
        self.names = [str(n) for n in self.z["names"]]

    def inputs(self, name):
        z = self.z
        return z[name + "/cell"], z[name + "/centers"], z[name + "/n_ij"], json.loads(str(z[name + "/kw"]))

    def expected(self, name):
        z = self.z
        return {k: z["%s/out_%s" % (name, k)] for k in ("codes", "labels", "site", "edge", "count", "dir_rows", "dir_offsets")}
