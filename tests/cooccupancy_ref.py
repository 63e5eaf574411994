"""Shared by tests/test_threshold_merge.py (CPU) and tests/test_gpu_cooccupancy.py (GPU): the brute-force co-occupancy
matrix, designed label sets, and the networks of the threshold goldens."""
import numpy as np

from tests import golden_util as G


def brute_cooccupancy(labels, n_sites):
    """The entries dynamics/MergeSitesByThreshold.py:64-70 clears: every pair of known sites of every frame."""
    labels = np.asarray(labels)
    if (labels >= n_sites).any():
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (labels[labels >= n_sites].min(), n_sites))
    co = np.zeros((n_sites, n_sites), dtype=bool)
    for frame in labels:
        known = frame[frame >= 0]
        co[np.ix_(known, known)] = True
    return co


def designed_labels(F, M, seed, p_stay=0.97, p_unknown=0.02):
    """Ion j lives on sites 4j .. 4j+3 of K = 4M + 3 sites (the last three are never visited): every frame it keeps its
    site with probability ``p_stay``, otherwise draws again among its four; then every entry independently becomes -1
    with probability ``p_unknown``.  Returns (labels[F, M], K)."""
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 4, size=M)
    lab = np.empty((F, M), dtype=np.int64)
    for f in range(F):
        again = rng.uniform(size=M) >= p_stay
        state = np.where(again, rng.integers(0, 4, size=M), state)
        lab[f] = 4 * np.arange(M) + state
    lab[rng.uniform(size=(F, M)) < p_unknown] = -1
    return lab, 4 * M + 3


def off_diagonal_fill(co):
    K = len(co)
    return co[~np.eye(K, dtype=bool)].mean() if K > 1 else 0.0


def plain_network(n_mobile, n_sites, seed=0):
    """A network of ``n_sites`` random centres in a 12 Angstrom cube with one static atom and ``n_mobile`` mobile ones."""
    from sitator_amd import SiteNetwork, Structure
    sm = np.array([True] + [False] * n_mobile)
    sn = SiteNetwork(Structure(np.zeros((n_mobile + 1, 3)), np.eye(3) * 12.0), sm, ~sm)
    sn.centers = np.random.default_rng(seed).uniform(0.0, 12.0, size=(n_sites, 3))
    return sn


class ThresholdGoldens(object):
    """tests/golden/threshold_known_answers.npz with the inputs it shares with merge_known_answers.npz."""

    def __init__(self):
        self.z = G.load("threshold_known_answers")
        self.src = G.load("merge_known_answers")
        self.names = [str(n) for n in self.z["names"]]
        self.variants = [str(v) for v in self.z["variants"]]

    def cases(self):
        return [(n, v) for n in self.names for v in self.variants]

    def labels(self, name):
        return self.src[name + "/labels"]

    def network(self, name, centers=None):
        from sitator_amd import SiteNetwork, Structure
        s = self.src
        sn = SiteNetwork(Structure(s[name + "/ref_positions"], s[name + "/cell"]), s[name + "/static_mask"],
                         s[name + "/mobile_mask"])
        sn.centers = np.array(s[name + "/centers"] if centers is None else centers, copy=True)
        return sn

    def with_dead_sites(self, name):
        """The inputs of case (a) of RemoveUnoccupiedSites, rebuilt by the generator's rule: the sites ``dead`` are put
        in (centres: the first three centres + 0.1), the labels move to the remaining indices."""
        cen, lab = self.src[name + "/centers"], self.labels(name)
        dead = self.z[name + "/rm_a/dead"]
        alive = np.setdiff1d(np.arange(len(cen) + 3), dead)
        centers = np.empty((len(cen) + 3, 3))
        centers[alive] = cen
        centers[dead] = cen[:3] + 0.1
        return centers, np.where(lab >= 0, alive[np.where(lab >= 0, lab, 0)], -1)


def attach_jump_statistics(oracle, st):
    """n_ij / p_ij / jump_lag of the CPU oracle's JumpAnalysis as edge attributes (where no device computes them)."""
    sn = st.site_network
    ja = oracle.jump_analysis(np.asarray(st._traj), sn.n_sites)
    for attr in ("n_ij", "p_ij", "jump_lag"):
        sn.add_edge_attribute(attr, np.asarray(ja[attr]))


def run_threshold_variant(st, params):
    """Runs MergeSitesByThreshold as the golden's ``params`` say; returns (error class name or "", result)."""
    import operator
    from sitator_amd import MergeSitesByThreshold, MergedSitesTooDistantError, errors
    op = MergeSitesByThreshold(params["attrname"], relation=getattr(operator, params["relation"]), check_types=False,
                               **params["kw"])
    try:
        return "", op.run(st, threshold=params["threshold"])
    except (MergedSitesTooDistantError, errors.InsufficientSitesError) as e:
        return type(e).__name__, None


def sharded_labels():
    """A designed label set for frame shards, with the cuts for 2 and 3 ranks.  Rank 1 starts at frame 40 in both; ion 0
    sits on the spare site K-3 in frame 40 only (pairs with K-3 exist in no other frame), ion 1 on the spare site K-2 in
    frame 88 only (the last rank's), and K-1 is never visited."""
    lab, K = designed_labels(90, 6, seed=11)
    lab[40, :] = np.where(lab[40] < 0, 4 * np.arange(6), lab[40])      # everybody known in the frame that matters
    lab[40, 0] = K - 3
    lab[88, 1] = K - 2
    return lab, K, {2: [0, 40, 90], 3: [0, 40, 70, 90]}


def run_sharded(oracle, lab, K, cut):
    """(single-rank results, per-rank results in rank order, exceptions).  A result: (co, merged st, pruned st, kept)."""
    import threading
    from sitator_amd import MergeSitesByThreshold, RemoveUnoccupiedSites, SiteTrajectory
    from sitator_amd.sharding import ThreadComm
    n_ij = np.asarray(oracle.jump_analysis(lab, K)["n_ij"])

    def work(st):
        st.site_network.add_edge_attribute("n_ij", n_ij.copy())
        co = st.compute_site_cooccupancy()
        merged = MergeSitesByThreshold("n_ij", forbid_multiple_occupancy=True, check_types=False).run(st, threshold=1)
        pruned, kept = RemoveUnoccupiedSites().run(st, return_kept_sites=True)
        return co, merged, pruned, kept[0]

    single = work(SiteTrajectory(plain_network(lab.shape[1], K), lab))
    comms = ThreadComm.group(len(cut) - 1)
    joined, failures = [None] * len(comms), []

    def rank(r):
        try:
            joined[r] = work(SiteTrajectory(plain_network(lab.shape[1], K), lab[cut[r]:cut[r + 1]], _comm=comms[r]))
        except BaseException as e:                               # noqa: BLE001 - reported by the caller
            failures.append((r, repr(e)))
            comms[r].abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(len(comms))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return single, joined, failures


def compare_sharded(single, joined, lab, K):
    co, merged, pruned, kept = single
    assert np.array_equal(co, brute_cooccupancy(lab, K))
    assert np.array_equal(kept, np.unique(lab[lab >= 0])) and len(kept) < K
    assert K - 2 in kept and K - 1 not in kept                    # K-2 (last rank only) stays, K-1 goes
    assert merged.site_network.n_sites < K
    for part in joined:
        assert np.array_equal(part[0], co)
        assert np.array_equal(part[3], kept)
        assert np.array_equal(np.asarray(part[1].site_network.centers), np.asarray(merged.site_network.centers))
        assert np.array_equal(np.asarray(part[2].site_network.centers), np.asarray(pruned.site_network.centers))
    assert np.array_equal(np.concatenate([p[1].traj for p in joined]), merged.traj)
    assert np.array_equal(np.concatenate([p[2].traj for p in joined]), pruned.traj)
