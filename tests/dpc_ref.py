"""TEST INFRASTRUCTURE: density-peak clustering (Rodriguez & Laio, Science 344, 1492 (2014)) restated in numpy the way
``pydpc.Cluster`` is laid out - a dense N x N float64 distance matrix, a sort of its upper triangle for the kernel size, loops
for delta and membership - with the definitions of ``sitator_amd/csrc/dpc_plan.h``.  Small N only.

The distance follows the header's order (ascending coordinate, every operation rounded on its own; numpy does not contract), so
``distances`` reproduces the header's bytes: the kernel size, delta and neighbour can be compared exactly."""
import numpy as np


def distances(Y):
    Y = np.asarray(Y, dtype=np.float64)
    s = np.zeros((len(Y), len(Y)))
    for k in range(Y.shape[1]):
        t = Y[:, None, k] - Y[None, :, k]
        s = s + t * t
    return np.sqrt(s)


def rank_of(n, fraction):
    return min(int(np.floor(0.5 + fraction * float(n))), n - 1)


def kernel_size(dist, fraction):
    """``(dc, rank, n)``: the element of rank ``min(floor(0.5 + fraction n), n - 1)`` of the sorted distances ``i < j``."""
    iu = np.triu_indices(len(dist), k=1)
    upper = np.sort(dist[iu])
    n = len(upper)
    r = rank_of(n, fraction)
    return upper[r], r, n


def weights(dist, dc):
    if dc > 0.0:
        with np.errstate(over="ignore"):
            q = dist / dc
            return np.exp(-(q * q))
    return (dist == 0.0).astype(np.float64)


def density(dist, dc):
    """``rho_i = sum_{j != i} w(d_ij)`` in numpy's summation order (the device's order differs: the comparison is within the
    bound of a reordered sum of positive terms)."""
    w = weights(dist, dc)
    np.fill_diagonal(w, 0.0)
    return np.sum(w, axis=1)


def delta_neighbour(dist, rho):
    """The plan's rule, a point at a time: ``j`` is above ``i`` iff ``rho_j > rho_i``, or they are equal and ``j < i``;
    ``delta_i`` = the smallest distance to a point above ``i``; of equal distances the highest point wins; the top point gets -1
    and the largest delta of the others."""
    rho = np.asarray(rho, dtype=np.float64)
    N = len(rho)
    delta = np.zeros(N)
    nbr = np.full(N, -1, dtype=np.int32)
    index = np.arange(N)
    for i in range(N):
        cand = np.where((rho > rho[i]) | ((rho == rho[i]) & (index < i)))[0]          # the points above i
        if len(cand) == 0:
            continue
        nearest = cand[dist[i, cand] == np.min(dist[i, cand])]
        densest = nearest[rho[nearest] == np.max(rho[nearest])]
        nbr[i] = densest[0]                                                            # ascending: the smallest index of those
        delta[i] = dist[i, nbr[i]]
    top = np.where(nbr < 0)[0]
    assert len(top) == 1
    delta[top[0]] = np.max(delta[nbr >= 0])
    return delta, nbr


def order_of(rho):
    """Densest first, equal densities by ascending index."""
    return np.lexsort((np.arange(len(rho)), -np.asarray(rho))).astype(np.int32)


def assign(rho, delta, nbr, min_density, min_delta):
    """``(membership, clusters)``: centres numbered in ascending index, every other point follows its neighbour; a chain that
    ends at a point that is no centre and has no neighbour gives -1."""
    N = len(rho)
    centre = (rho > min_density) & (delta > min_delta)
    clusters = np.where(centre)[0].astype(np.int32)
    number = np.full(N, -1, dtype=np.int32)
    number[clusters] = np.arange(len(clusters), dtype=np.int32)
    membership = np.full(N, -1, dtype=np.int32)
    for i in range(N):
        k, steps = i, 0
        while not centre[k] and nbr[k] >= 0 and steps <= N:
            k, steps = nbr[k], steps + 1
        membership[i] = number[k] if centre[k] else -1
    return membership, clusters


def votes(membership, dvecs_to_site, K, n_clusters):
    v = np.zeros((K, n_clusters), dtype=np.int64)
    for m, s in zip(membership, dvecs_to_site):
        if m >= 0:
            v[s, m] += 1
    return v


class Cluster(object):
    """The surface of ``pydpc.Cluster`` that ``SiteTypeAnalysis`` touches, on the loops above."""

    def __init__(self, points, fraction=0.02, autoplot=True):
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.npoints = len(self.points)
        self.fraction = fraction
        self.distances = distances(self.points)
        self.kernel_size = kernel_size(self.distances, fraction)[0]
        self.density = density(self.distances, self.kernel_size)
        self.delta, self.neighbour = delta_neighbour(self.distances, self.density)
        self.order = order_of(self.density)

    def assign(self, min_density, min_delta, border_only=False):
        self.min_density, self.min_delta = min_density, min_delta
        self.membership, self.clusters = assign(self.density, self.delta, self.neighbour, min_density, min_delta)
        self.nclusters = len(self.clusters)
