"""CPU-only: ``ConfigurationalEntropy`` against what the reference's own file returned on the label arrays of
tests/entropy_ref.py (tests/golden/entropy_known_answers.npz, recorded by tests/make_entropy_golden.py) and against the numpy
restatement.  The residences are put on the network from ``entropy_ref.residences``, so ``compute`` runs no ``JumpAnalysis``
and needs no GPU; tests/test_gpu_coordenv.py runs the branch that does."""
import json

import numpy as np
import pytest

from tests import entropy_ref as ER
from tests.make_entropy_golden import network

CASES = ER.cases()


@pytest.fixture(scope="module")
def golden():
    g = np.load(ER.GOLDEN)
    assert json.loads(str(g["names"])) == list(CASES)
    return g


@pytest.mark.parametrize("name", sorted(CASES))
def test_compute_is_the_reference(golden, name):
    from sitator_amd import ConfigurationalEntropy
    labels, n_sites, site_types, overshoot = CASES[name]
    assert labels.shape[0] <= 64 and labels.shape[1] <= 8
    assert np.array_equal(golden[name + "/labels"], labels)
    st = network(labels, n_sites, site_types)
    op = ConfigurationalEntropy(acceptable_overshoot=overshoot)
    if name + "/raises" in golden.files:
        with pytest.raises(ValueError) as err:
            op.compute(st)
        assert str(err.value) == str(golden[name + "/raises"])
        return
    got, ref = op.compute(st), float(golden[name + "/expected"][0])
    assert abs(got - ref) <= 1e-12 * abs(ref)
    if "overshoot" not in name:
        mine = ER.entropy(ER.residences(labels, n_sites), len(labels), site_types)
        assert abs(got - mine) <= 1e-12 * abs(mine)


def test_the_cases_cover_both_branches_and_both_outcomes(golden):
    raised = [n for n in CASES if n + "/raises" in golden.files]
    assert sorted(raised) == ["by_site_overshoot_not_forgiven", "by_site_overshoot_raises", "by_type_overshoot_raises"]
    assert any(CASES[n][2] is None for n in CASES) and any(CASES[n][2] is not None for n in CASES)
    assert any((CASES[n][0] < 0).any() for n in CASES)
    assert float(golden["by_site_overshoot_forgiven/expected"][0]) == 0.0


def test_s_tilde(golden):
    from sitator_amd import ConfigurationalEntropy
    got = ConfigurationalEntropy().s_tilde(golden["s_tilde/p2"].copy(), float(golden["s_tilde/n"][0]), golden["s_tilde/N"])
    ref = float(golden["s_tilde/expected"][0])
    assert abs(got - ref) <= 1e-12 * abs(ref)
    assert ConfigurationalEntropy().s_tilde(np.array([0.0, 1.0]), 1.0, np.array([2, 3])) == 0.0
    assert abs(ConfigurationalEntropy().s_tilde(np.array([0.5]), 2.0, np.array([4])) - 2.0 * np.log(2.0)) <= 1e-15


def test_frame_shard_is_refused():
    from sitator_amd import ConfigurationalEntropy

    class TwoRanks(object):
        size, rank = 2, 0
    labels, n_sites, site_types, _ = CASES["by_site_few_frames"]
    st = network(labels, n_sites, site_types)
    st._comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        ConfigurationalEntropy().compute(st)
