"""GPU: ``k_cooccupancy`` (sites.hip) and the operators on top of it - ``SiteTrajectory.compute_site_cooccupancy``,
``MergeSitesByThreshold``, ``RemoveUnoccupiedSites`` - against the reference's goldens
(tests/golden/threshold_known_answers.npz) and against numpy brute force on designed and hand-built label sets.

The kernel pairs only the ions whose label CHANGED against the frame before (every known ion in the context's frame 0)
with the known ions of their frame; a workgroup takes ``BLOCK`` consecutive frames, a wave of it every fourth, the ions
in groups of 64 lanes.  What that can get wrong is planted below: pairs that exist in one frame only (frame 0, a frame
entered from -1, the first frame of every workgroup block and its neighbours), M above 64 and above 128, M = 1, a
ragged last block, K that is no multiple of 64."""
import json

import numpy as np
import pytest

from tests import cooccupancy_ref as R

pytestmark = pytest.mark.gpu

BLOCK = 64                                           # CO_FRAMES_PER_WG of sites.hip
TG = R.ThresholdGoldens()


def device_cooccupancy(labels, K):
    from sitator_amd import _lib
    ctx = _lib.HipContext(np.eye(3) * 10.0)
    try:
        ctx.set_assignments(np.asarray(labels, dtype=np.int64))
        return ctx.cooccupancy(K)
    finally:
        ctx.close()


# ---- 1. the reference's goldens through the real context ------------------------------------------------------------

@pytest.mark.parametrize("name,variant", TG.cases())
def test_gpu_merge_by_threshold_matches_reference(name, variant):
    from sitator_amd import JumpAnalysis, SiteTrajectory
    key = "%s/%s" % (name, variant)
    params = json.loads(str(TG.z[key + "/params"]))
    st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
    JumpAnalysis().run(st)
    err, out = R.run_threshold_variant(st, params)
    assert err == str(TG.z[key + "/error"])
    if not err:
        assert np.array_equal(out.traj, TG.z[key + "/traj"])
        np.testing.assert_allclose(np.asarray(out.site_network.centers), TG.z[key + "/centers"], rtol=1e-6, atol=1e-9)
        assert out.site_network.n_sites == len(TG.z[key + "/centers"])


@pytest.mark.parametrize("name", TG.names)
def test_gpu_cooccupancy_and_removal_match_reference(name):
    from sitator_amd import RemoveUnoccupiedSites, SiteTrajectory, errors
    z, key = TG.z, name + "/rm_a"
    st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
    co = st.compute_site_cooccupancy()
    assert co.dtype == np.bool_ and np.array_equal(co, z[name + "/cooccupancy"])
    assert RemoveUnoccupiedSites().run(st, return_kept_sites=True) is st
    centers, labels = TG.with_dead_sites(name)
    sn = TG.network(name, centers)
    sn.site_types = z[key + "/in_types"]
    sn.add_site_attribute("score", z[key + "/in_score"])
    sn.add_edge_attribute("weight", z[key + "/in_weight"])
    out, kept = RemoveUnoccupiedSites().run(SiteTrajectory(sn, labels), return_kept_sites=True)
    assert np.array_equal(kept[0], z[key + "/kept"]) and np.array_equal(out.traj, z[key + "/traj"])
    new = out.site_network
    np.testing.assert_allclose(np.asarray(new.centers), z[key + "/centers"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(new.site_types, z[key + "/types"])
    assert np.array_equal(new.score, z[key + "/score"]) and np.array_equal(new.weight, z[key + "/weight"])
    lab = TG.labels(name)
    folded = np.where(lab >= 0, lab % int(z[name + "/rm_c/modulus"]), -1)
    with pytest.raises(errors.InsufficientSitesError):
        RemoveUnoccupiedSites().run(SiteTrajectory(TG.network(name), folded))


# ---- 2. designed labels against brute force -------------------------------------------------------------------------

@pytest.mark.parametrize("F,M", [(131, 70), (259, 5), (67, 130), (131, 1)])
def test_designed_labels_bit_equal_to_brute_force(F, M):
    lab, K = R.designed_labels(F, M, seed=5)
    assert K % 64 != 0 and F % BLOCK != 0 and F > BLOCK
    exp = R.brute_cooccupancy(lab, K)
    fill = R.off_diagonal_fill(exp)
    print("F=%d M=%d K=%d: %.1f%% of the off-diagonal set" % (F, M, K, 100.0 * fill))
    if M > 1:
        assert 0.15 < fill < 0.85                    # neither empty nor saturated: agreement means something
    else:
        visited = np.zeros(K, dtype=bool)
        visited[lab[lab >= 0]] = True
        assert np.array_equal(exp.diagonal(), visited) and visited.any() and fill == 0.0
    got = device_cooccupancy(lab, K)
    assert got.dtype == np.bool_ and got.shape == (K, K)
    assert np.array_equal(got, exp)
    assert np.array_equal(got, got.T)


# ---- 3. hand-built cases: first the brute-force matrix is asserted, then the device's equals it ------------------------

def _only_frame_0():
    lab = np.array([[0, 1], [0, -1], [0, -1], [-1, 2], [0, -1]])
    return lab, 4, [(0, 1, True), (1, 0, True), (0, 2, False), (1, 2, False), (2, 2, True), (3, 3, False)]


def _newcomer_from_unknown():
    lab = np.array([[3, -1], [3, -1], [3, 4], [3, -1], [-1, 4]])
    return lab, 6, [(3, 4, True), (4, 3, True), (4, 4, True), (3, 3, True), (0, 0, False)]


def _changes_on_block_starts():
    """Ion 0 never moves (site 0).  Ion 1 leaves site 1 for ONE frame at every index that begins a block of BLOCK frames
    (sites 10, 11, 12), at the last frame of a block (13) and at the second frame of one (14).  Ion 2 moves for good at a
    block start (2 -> 20).  F = 3 * BLOCK + 5: the last block is ragged."""
    F = 3 * BLOCK + 5
    lab = np.empty((F, 3), dtype=np.int64)
    lab[:, 0], lab[:, 1], lab[:, 2] = 0, 1, 2
    lab[BLOCK, 1], lab[2 * BLOCK, 1], lab[3 * BLOCK, 1] = 10, 11, 12
    lab[BLOCK - 1, 1], lab[2 * BLOCK + 1, 1] = 13, 14
    lab[2 * BLOCK:, 2] = 20
    checks = [(0, s, True) for s in (10, 11, 12, 13, 14, 20, 1, 2)]
    checks += [(10, 2, True), (10, 20, False), (11, 20, True), (11, 2, False), (12, 20, True), (13, 2, True),
               (14, 20, True), (14, 2, False), (1, 20, True), (10, 11, False), (2, 20, False), (15, 15, False)]
    return lab, 23, checks


def _two_ions_on_one_site():
    lab = np.array([[1, 2, 6], [5, 5, 6], [1, 2, -1]])
    return lab, 7, [(5, 5, True), (5, 6, True), (6, 5, True), (1, 5, False), (2, 5, False), (1, 2, True), (1, 6, True)]


def _an_ion_never_assigned():
    lab = np.array([[0, -1, 1], [2, -1, 1], [2, -1, 3]])
    return lab, 5, [(0, 1, True), (2, 1, True), (2, 3, True), (0, 3, False), (0, 2, False), (4, 4, False)]


def _nobody_assigned():
    return np.full((BLOCK + 3, 5), -1, dtype=np.int64), 9, []


def _three_sites():
    lab = np.array([[0, 1], [2, -1], [2, 2]])
    return lab, 3, [(0, 1, True), (1, 0, True), (2, 2, True), (0, 2, False), (1, 2, False), (0, 0, True)]


HAND_BUILT = [_only_frame_0, _newcomer_from_unknown, _changes_on_block_starts, _two_ions_on_one_site,
              _an_ion_never_assigned, _nobody_assigned, _three_sites]


@pytest.mark.parametrize("case", HAND_BUILT, ids=[c.__name__.strip("_") for c in HAND_BUILT])
def test_hand_built_cases(case):
    lab, K, checks = case()
    exp = R.brute_cooccupancy(lab, K)
    for a, b, value in checks:
        assert exp[a, b] == value, (a, b)
    if not checks:
        assert not exp.any()
    got = device_cooccupancy(lab, K)
    for a, b, value in checks:
        assert got[a, b] == value, (a, b)
    assert np.array_equal(got, exp)


def test_a_label_beyond_the_sites_raises_index_error():
    lab, K, _ = _changes_on_block_starts()
    lab[BLOCK + 7, 1] = K
    with pytest.raises(IndexError):
        R.brute_cooccupancy(lab, K)
    with pytest.raises(IndexError, match="index %d is out of bounds" % K):
        device_cooccupancy(lab, K)


def test_no_frames_give_an_empty_matrix():
    got = device_cooccupancy(np.zeros((0, 3), dtype=np.int64), 5)
    assert got.shape == (5, 5) and not got.any()


# ---- 4. frame shards ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_gpu_frame_shards_equal_the_single_rank(oracle, n):
    """``ThreadComm.group(n)``, a thread and a context per rank on GPU 0, contiguous frame blocks.  One pair exists only in
    the first frame of rank 1 (asserted on numpy by deleting that frame), one site is visited on the last rank only."""
    lab, K, cuts = R.sharded_labels()
    first_of_rank_1 = cuts[n][1]
    assert R.brute_cooccupancy(lab, K)[K - 3].any()
    assert not R.brute_cooccupancy(np.delete(lab, first_of_rank_1, axis=0), K)[K - 3].any()
    assert (lab[cuts[n][-2]:] == K - 2).any() and not (lab[:cuts[n][-2]] == K - 2).any()
    single, joined, failures = R.run_sharded(oracle, lab, K, cuts[n])
    assert not failures, failures
    R.compare_sharded(single, joined, lab, K)


# ---- 5. after the landmark path: the labels are read where run() left them --------------------------------------------

def test_operators_read_the_labels_where_run_left_them():
    from sitator_amd import (JumpAnalysis, LandmarkAnalysis, MergeSitesByThreshold, RemoveUnoccupiedSites, SiteNetwork,
                             SiteTrajectory, Structure, synth, _lib)
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 500, seed=17, p_hop=1.0 / 40)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    st = LandmarkAnalysis(verbose=False).run(sn, frames)

    def pipeline(s):
        JumpAnalysis().run(s)
        co = s.compute_site_cooccupancy()
        pruned = RemoveUnoccupiedSites().run(s)
        merged = MergeSitesByThreshold("n_ij", forbid_multiple_occupancy=True, check_types=False).run(s, threshold=1)
        return co, pruned, merged

    uploads = []
    real = _lib.HipContext.set_assignments

    def counting(self, *a, **k):
        uploads.append(1)
        return real(self, *a, **k)

    _lib.HipContext.set_assignments = counting
    try:
        co, pruned, merged = pipeline(st)
        assert len(uploads) == 0, "the labels run() left on the device must not be uploaded again"
    finally:
        _lib.HipContext.set_assignments = real
    fresh = SiteTrajectory(st.site_network.copy(), st.traj.copy())
    fresh.site_network.clear_attributes()
    co2, pruned2, merged2 = pipeline(fresh)
    final, final2 = RemoveUnoccupiedSites().run(merged), RemoveUnoccupiedSites().run(merged2)
    assert np.array_equal(co, co2) and np.array_equal(co, R.brute_cooccupancy(st.traj, st.site_network.n_sites))
    assert merged.site_network.n_sites < st.site_network.n_sites
    for a, b in ((pruned, pruned2), (merged, merged2), (final, final2)):
        assert np.array_equal(a.traj, b.traj)
        assert np.array_equal(np.asarray(a.site_network.centers), np.asarray(b.site_network.centers))
