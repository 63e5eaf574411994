"""CPU: the host logic of ``ReplaceUnassignedPositions`` against goldens of the TRUE reference
(tests/golden/replace_unassigned_known_answers.npz, written by tools/make_replace_goldens.py), the ``with_computed``
copies of ``SiteNetwork`` / ``SiteTrajectory`` and the derivation of a frame shard's carried-in values.  The device is
replaced by a test double that serves the four label calls by brute force (tests/replace_ref.py); the kernels themselves
are covered by tests/test_gpu_replace_unassigned.py."""
import numpy as np
import pytest

from tests import replace_ref as R
from tests.fake_ctx import FakeContext

RG = R.ReplaceGoldens()


class ReplaceFakeContext(FakeContext):
    ENDS_NONE = R.NONE

    def _lab(self):
        return self._labels.reshape(self.F, self.M)

    def label_ends(self):
        return R.ends(self._lab())

    def replace_unassigned(self, mode, before_in=None, after_in=None):
        return R.replace(self._lab(), mode, before_in, after_in)

    def unknown_runs(self, before_in=None, after_in=None):
        return R.runs(self._lab(), before_in, after_in, self.frame0)

    def replace_closer(self, records, centers, positions):
        out = self._lab().copy()
        for j, s, e, b, a, off in records:
            if max(b, a) >= len(centers):
                raise IndexError("index %d is out of bounds for axis 0 with size %d" % (max(b, a), len(centers)))
            if b < 0 or a < 0:
                continue
            for i, f in enumerate(range(s - self.frame0, e - self.frame0)):
                if b == a:
                    out[f, j] = b
                else:
                    d = self.distances(positions[off + i], np.asarray(centers)[[b, a]])
                    out[f, j] = b if d[0] < d[1] else a
        return out


@pytest.fixture
def fake_device(monkeypatch):
    from sitator_amd import _lib, pbc
    monkeypatch.setattr(_lib, "HipContext", ReplaceFakeContext)
    monkeypatch.setattr(pbc, "HipContext", ReplaceFakeContext)


def test_brute_force_agrees_with_the_reference_on_the_goldens():
    """The brute force the GPU tests compare the kernels with, pinned to the reference first."""
    for name in RG.names:
        lab = RG.inputs(name)["labels"]
        assert np.array_equal(R.replace(lab, 0), RG.z[name + "/last"])
        assert np.array_equal(R.replace(lab, 1), RG.z[name + "/next"])
        rec, npos = R.runs(lab)
        assert np.array_equal(rec[:, [0, 3, 1, 4, 2]], RG.z[name + "/calls"])
        dec = rec[rec[:, 5] >= 0]
        assert npos == (dec[:, 2] - dec[:, 1]).sum()
        assert np.array_equal(dec[:, 5], np.concatenate([[0], np.cumsum(dec[:, 2] - dec[:, 1])[:-1]])[:len(dec)])


@pytest.mark.parametrize("name", RG.names)
def test_operator_matches_the_reference(fake_device, oracle, name):
    R.check_golden_case(RG, name, margin_oracle=oracle)


def test_brute_closer_agrees_with_the_reference(oracle):
    for name in RG.names:
        i = RG.inputs(name)
        out, margin = R.closer(oracle, i["cell"], i["labels"], i["centers"], RG.mobile_positions(name))
        assert np.array_equal(out, RG.z[name + "/closer"]) and margin >= R.MARGIN


def test_the_default_constructor_fills_with_the_last_known_site(fake_device):
    from sitator_amd import ReplaceUnassignedPositions as RUP, SiteTrajectory
    assert RUP().replacement_function is RUP.replace_with_last_known
    assert RUP.replace_with_last_known(None, 0, 3, 1, 4, 2) == 3 and RUP.replace_with_next_known(None, 0, 3, 1, 4, 2) == 4
    lab = np.array([[-1, 2], [1, -1], [-1, -1], [3, 0]])
    out = RUP().run(SiteTrajectory(R.plain_network(2, np.zeros((4, 3))), lab))
    assert np.array_equal(out.traj, [[-1, 2], [1, 2], [1, 2], [3, 0]])


def test_closer_callable_on_its_own(fake_device):
    """The factory's callable, as a plain callable: an unknown neighbour gives SITE_UNKNOWN, a far centre that is near
    through a periodic image wins, a tie goes to the site after, no real trajectory is a ValueError."""
    from sitator_amd import ReplaceUnassignedPositions as RUP, SiteTrajectory
    cell = np.eye(3) * 10.0
    centers = np.array([[4.0, 5.0, 5.0], [9.5, 5.0, 5.0], [2.0, 5.0, 5.0], [2.0, 5.0, 5.0]])
    st = SiteTrajectory(R.plain_network(1, centers, cell), np.array([[0], [-1], [-1], [-1], [1]]))
    fn = RUP.replace_with_closer()
    assert callable(fn)
    assert fn(st, 0, -1, 1, 1, 4) == SiteTrajectory.SITE_UNKNOWN and fn(st, 0, 0, 1, -1, 4) == SiteTrajectory.SITE_UNKNOWN
    with pytest.raises(ValueError):
        fn(st, 0, 0, 1, 1, 4)
    pos = np.zeros((5, 1, 3))
    pos[:, 0] = [[4, 5, 5], [0.5, 5, 5], [3.0, 5, 5], [1.0, 5, 5], [9.5, 5, 5]]
    st.set_real_traj(R.real_trajectory(pos))
    # x = 0.5 is 3.5 from site 0 and 1.0 from site 1 through the cell's face; x = 3.0: 1.0 against 3.5; x = 1.0: 3.0 / 1.5
    assert np.array_equal(fn(st, 0, 0, 1, 1, 4), [1, 0, 1])
    # sites 2 and 3 share their centre, the same distance bit for bit: the site AFTER the run takes the frame
    assert np.array_equal(fn(st, 0, 2, 2, 3, 3), [3]) and np.array_equal(fn(st, 0, 3, 2, 2, 3), [2])
    assert np.array_equal(RUP(fn).run(st).traj[:, 0], [0, 1, 0, 1, 1])


def test_any_other_callable_on_frame_shards_is_refused(fake_device):
    single, joined, failures = R.run_sharded(*R.sharded_case()[:3], [0, 40, 90], custom=True)
    assert sorted(failures) == [(0, "NotImplementedError"), (1, "NotImplementedError")]
    assert np.array_equal(single[0], R.replace(R.sharded_case()[0], 0))


def test_with_computed_on_site_network_and_site_trajectory():
    from sitator_amd import SiteTrajectory
    sn = R.plain_network(2, np.arange(12.0).reshape(4, 3))
    sn.add_site_attribute("plain", np.arange(4), computed=False)
    sn.add_site_attribute("derived", np.arange(4) * 2.0)                   # computed is the default
    sn.add_edge_attribute("edge_plain", np.ones((4, 4)), computed=False)
    sn.add_edge_attribute("edge_derived", np.zeros((4, 4)), computed=True)
    full = sn.copy()
    assert sorted(full.site_attributes + full.edge_attributes) == ["derived", "edge_derived", "edge_plain", "plain"]
    lean = sn.copy(with_computed=False)
    assert lean.site_attributes == ["plain"] and lean.edge_attributes == ["edge_plain"]
    assert np.array_equal(lean.plain, np.arange(4)) and lean.plain is not sn.plain
    # the mark survives a copy and a subset: clearing the copy's computed attributes leaves the plain ones
    full.clear_computed_attributes()
    assert full.site_attributes == ["plain"] and full.edge_attributes == ["edge_plain"]
    part = sn[[0, 2]]
    part.clear_computed_attributes()
    assert part.site_attributes == ["plain"] and part.edge_attributes == ["edge_plain"]
    # removing and adding again takes the new mark
    sn.remove_attribute("plain")
    sn.add_site_attribute("plain", np.arange(4))
    sn.clear_computed_attributes()
    assert sn.site_attributes == [] and sn.edge_attributes == ["edge_plain"]
    sn.clear_attributes()
    sn.clear_computed_attributes()
    assert sn.edge_attributes == []
    sn.add_site_attribute("plain", np.arange(4), computed=False)
    sn.add_site_attribute("derived", np.arange(4))
    st = SiteTrajectory(sn, np.zeros((3, 2), dtype=np.int64))
    assert st.copy().site_network.site_attributes == ["plain", "derived"]
    lean = st.copy(with_computed=False)
    assert lean.site_network.site_attributes == ["plain"] and lean.site_network is not sn
    assert np.array_equal(lean.traj, st.traj) and sn.site_attributes == ["plain", "derived"]


@pytest.mark.parametrize("n", [2, 3])
def test_shard_halo_from_the_gathered_ends(n):
    """Every shard's carried-in values from the table of all shards' ends equal a search of the whole array - also for
    the ion that has no known label in the whole middle shard, the ion that is never known and the run over both cuts."""
    from sitator_amd.dynamics import shard_halo
    lab, _, _, cuts = R.sharded_case()
    cut = cuts[n]
    table = [R.ends(lab[cut[r]:cut[r + 1]]) for r in range(n)]
    first, last = np.array([t[0] for t in table]), np.array([t[1] for t in table])
    if n == 3:
        assert first[1, 2] == R.NONE and last[1, 2] == R.NONE
    assert (first[:, 3] == R.NONE).all()
    for r in range(n):
        b, a = shard_halo(first, last, r, R.NONE)
        eb, ea = R.shard_halo_brute(lab, cut, r)
        assert np.array_equal(b, eb) and np.array_equal(a, ea)
        assert b[3] == -1 and a[3] == -1
    if n == 3:
        b, a = shard_halo(first, last, 1, R.NONE)
        assert (b[4], a[4]) == (1, 5)
        b2, a0 = shard_halo(first, last, 2, R.NONE)[0], shard_halo(first, last, 0, R.NONE)[1]
        assert b2[2] == last[0, 2] and a0[2] == first[2, 2]                 # over the empty middle shard


@pytest.mark.parametrize("n", [2, 3])
def test_frame_shards_equal_the_single_rank(fake_device, n):
    lab, centers, pos, cuts = R.sharded_case()
    single, joined, failures = R.run_sharded(lab, centers, pos, cuts[n])
    assert not failures, failures
    assert np.array_equal(single[0], R.replace(lab, 0)) and np.array_equal(single[1], R.replace(lab, 1))
    assert (single[2] != single[0]).any() and (single[2] != single[1]).any()
    for k in range(3):
        assert np.array_equal(np.concatenate([part[k] for part in joined]), single[k]), k
