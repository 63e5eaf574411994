"""CPU: the host logic of ``MergeSitesByThreshold``, ``RemoveUnoccupiedSites`` and
``SiteTrajectory.compute_site_cooccupancy`` against goldens of the TRUE reference
(tests/golden/threshold_known_answers.npz, written by tools/make_threshold_goldens.py).  The device is replaced by the
oracle-backed test double with a brute-force ``cooccupancy``; the kernel itself is covered by
tests/test_gpu_cooccupancy.py."""
import json

import numpy as np
import pytest

from tests import cooccupancy_ref as R
from tests.fake_ctx import FakeContext

TG = R.ThresholdGoldens()


class CoFakeContext(FakeContext):
    def cooccupancy(self, K):
        return R.brute_cooccupancy(self._labels.reshape(self.F, self.M), int(K))


@pytest.fixture
def fake_device(monkeypatch):
    from sitator_amd import _lib, pbc
    monkeypatch.setattr(_lib, "HipContext", CoFakeContext)
    monkeypatch.setattr(pbc, "HipContext", CoFakeContext)


def _trajectory(name, oracle):
    from sitator_amd import SiteTrajectory
    st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
    R.attach_jump_statistics(oracle, st)
    return st


@pytest.mark.parametrize("name,variant", TG.cases())
def test_merge_by_threshold_matches_reference(fake_device, oracle, name, variant):
    key = "%s/%s" % (name, variant)
    params = json.loads(str(TG.z[key + "/params"]))
    st = _trajectory(name, oracle)
    before = {a: np.array(getattr(st.site_network, a), copy=True) for a in ("n_ij", "p_ij", "jump_lag")}
    err, out = R.run_threshold_variant(st, params)
    assert err == str(TG.z[key + "/error"])
    for a, v in before.items():                                   # the operator works on a copy of the attribute
        assert np.array_equal(getattr(st.site_network, a), v)
    if not err:
        assert np.array_equal(out.traj, TG.z[key + "/traj"])
        np.testing.assert_allclose(np.asarray(out.site_network.centers), TG.z[key + "/centers"], rtol=1e-9, atol=1e-9)
        assert out.confidences is None


@pytest.mark.parametrize("name", TG.names)
def test_cooccupancy_matches_the_generators_loop(fake_device, name):
    from sitator_amd import SiteTrajectory
    st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
    co = st.compute_site_cooccupancy()
    assert co.dtype == np.bool_ and np.array_equal(co, TG.z[name + "/cooccupancy"])
    assert st.site_network.site_attributes == [] and st.site_network.edge_attributes == []   # nothing stored


def test_cooccupancy_of_a_network_without_sites(fake_device):
    from sitator_amd import SiteNetwork, SiteTrajectory, Structure
    sm = np.array([True, False, False])
    sn = SiteNetwork(Structure(np.zeros((3, 3)), np.eye(3) * 5.0), sm, ~sm)
    co = SiteTrajectory(sn, np.full((4, 2), -1)).compute_site_cooccupancy()
    assert co.shape == (0, 0) and co.dtype == np.bool_


def test_merge_by_threshold_refuses_a_site_attribute(fake_device, oracle):
    from sitator_amd import MergeSitesByThreshold
    st = _trajectory("bcc_ortho", oracle)
    st.site_network.add_site_attribute("score", np.arange(st.site_network.n_sites))
    with pytest.raises(AssertionError, match="edge property"):
        MergeSitesByThreshold("score", check_types=False).run(st, threshold=1)


@pytest.mark.parametrize("name", TG.names)
def test_remove_unoccupied_sites_matches_reference(fake_device, name):
    from sitator_amd import RemoveUnoccupiedSites, SiteTrajectory, errors
    z, key = TG.z, name + "/rm_a"
    # (a) three never-visited sites; types, a site attribute, an edge attribute and (known answer) ragged vertices
    centers, labels = TG.with_dead_sites(name)
    sn = TG.network(name, centers)
    sn.site_types = z[key + "/in_types"]
    sn.add_site_attribute("score", z[key + "/in_score"])
    sn.add_edge_attribute("weight", z[key + "/in_weight"])
    vertices = [list(range(i, i + 1 + i % 3)) for i in range(sn.n_sites)]
    sn.vertices = vertices
    st = SiteTrajectory(sn, labels, confidences=np.ones(labels.shape))
    real = np.zeros((len(labels), sn.n_total, 3))
    st.set_real_traj(real)
    out, kept = RemoveUnoccupiedSites().run(st, return_kept_sites=True)
    assert isinstance(kept, tuple) and len(kept) == 1 and np.array_equal(kept[0], z[key + "/kept"])
    assert np.array_equal(np.setdiff1d(np.arange(sn.n_sites), kept[0]), z[key + "/dead"])
    assert np.array_equal(out.traj, z[key + "/traj"])
    new = out.site_network
    np.testing.assert_allclose(np.asarray(new.centers), z[key + "/centers"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(new.site_types, z[key + "/types"])
    assert np.array_equal(new.score, z[key + "/score"]) and np.array_equal(new.weight, z[key + "/weight"])
    assert new.vertices == [vertices[i] for i in kept[0]]
    assert out.confidences is None and out.real_trajectory is real
    assert sn.n_sites == len(centers) and np.array_equal(st.traj, labels)         # the input is left as it was
    plain = RemoveUnoccupiedSites().run(st)
    assert np.array_equal(plain.traj, out.traj)
    # (b) nothing to remove: the argument itself, alone, also when the kept sites were asked for
    st_b = SiteTrajectory(TG.network(name), TG.labels(name).copy())
    assert bool(z[name + "/rm_b/same_object"]) and RemoveUnoccupiedSites().run(st_b, return_kept_sites=True) is st_b
    assert RemoveUnoccupiedSites().run(st_b) is st_b
    # (c) fewer visited sites than mobile ions
    lab = TG.labels(name)
    st_c = SiteTrajectory(TG.network(name), np.where(lab >= 0, lab % int(z[name + "/rm_c/modulus"]), -1))
    assert str(z[name + "/rm_c/error"]) == "InsufficientSitesError"
    with pytest.raises(errors.InsufficientSitesError) as ei:
        RemoveUnoccupiedSites().run(st_c)
    assert ei.value.n_sites == int(z[name + "/rm_c/modulus"]) and ei.value.n_mobile == st_c.site_network.n_mobile
    assert str(ei.value).startswith("Removing unoccupied sites resulted in only")


def test_designed_sets_decide_something():
    """What the GPU tests rely on, checked where it can be checked without a GPU: the designed label sets are neither
    empty nor saturated, and the sharded set has the frame and the site its docstring promises."""
    for (F, M), seed in zip(((131, 70), (259, 5), (67, 130)), (5, 5, 5)):
        lab, K = R.designed_labels(F, M, seed)
        assert 0.15 < R.off_diagonal_fill(R.brute_cooccupancy(lab, K)) < 0.85, (F, M)
    lab, K, cuts = R.sharded_labels()
    full = R.brute_cooccupancy(lab, K)
    without = R.brute_cooccupancy(np.delete(lab, cuts[2][1], axis=0), K)
    partner = lab[40, 3]
    assert full[K - 3, partner] and full[partner, K - 3] and not without[K - 3].any()
    assert cuts[2][1] == cuts[3][1] == 40
    for n in (2, 3):
        last = lab[cuts[n][-2]:]
        assert (last == K - 2).any() and not (lab[:cuts[n][-2]] == K - 2).any() and not (lab == K - 1).any()


@pytest.mark.parametrize("n", [2, 3])
def test_frame_shards_or_the_matrices_and_sum_the_counts(fake_device, oracle, n):
    """Contiguous frame blocks, a thread and a (fake) context per rank: the joined results of both operators equal the
    single-rank ones, although one pair exists only in rank 1's first frame and one site only on the last rank."""
    lab, K, cuts = R.sharded_labels()
    single, joined, failures = R.run_sharded(oracle, lab, K, cuts[n])
    assert not failures, failures
    R.compare_sharded(single, joined, lab, K)
